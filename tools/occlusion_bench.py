"""Time the visibility floor and the gated plane sweep on one GPU, and say what the gate does to the swept
DSM: the workload of tools/sweep_bench.py — the four shipped JAX_269 cameras and their downscale-4 images
over the lidar ROI (256 m square, UTM zone 17) on a 512 x 512 grid of 0.5 m, K = 64 planes from −30 m in
steps of 0.5 m, window radius 2.

Steps, each a fresh process under a time limit of its own; a step is not started when the one before it
fails:

* ``floor`` — ``visibility_floor`` of the lidar raster (tests/golden/dsm_truth.npz) under the four cameras'
  lines of sight: the two launches by the library's own timer (class "occlusion_floor") and the whole call;
* ``ungated`` / ``gated`` — ``plane_sweep`` and ``visible_sweep`` with every floor −inf, by the library's
  timer (classes "sweep" and "occlusion_sweep"), run as processes that alternate ``--rounds`` times;
  with ``--parent-lib NAME`` the ungated process loads that library (a build of the parent commit beside
  libspnerf_amd.so) instead of this tree's;
* ``real`` — ``visible_sweep`` with the lidar's floor, slack one step: its time and the share of the
  (view, cell, plane) triples the gate takes out;
* ``refine`` — ``refine_sweep`` as a whole call, from its own first pass and from the lidar as the prior,
  beside ``smooth_sweep``: the altitude MAE and the median |error| against the lidar raster.

    python tools/occlusion_bench.py [--calls 5] [--warmup 1] [--rounds 3] [--parent-lib NAME] [--out profiles/r23/occlusion.txt]
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

from sweep_bench import ALT_LO, PLANES, RADIUS, SIDE, STEP, scene   # noqa: E402

LIMITS = {"floor": 120, "ungated": 180, "gated": 180, "real": 180, "refine": 300}   # seconds per step


def lidar():
    gt = np.load(os.path.join(ROOT, "tests", "golden", "dsm_truth.npz"))["gt"].astype(np.float64)
    assert gt.shape == (SIDE, SIDE)
    return gt


def lidar_floor(dev):
    from spnerf_amd import rectify, visibility_floor
    images, cams, grid = scene(dev)
    dirs, spread = rectify.view_directions(grid, cams, ALT_LO, ALT_LO + (PLANES - 1) * STEP, dev)
    prior = torch.tensor(lidar(), device=dev)
    return images, cams, grid, prior, dirs, spread, visibility_floor(prior, grid, dirs)


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
    assert all(r["launches"] == 1 for r in k), k
    return [r["ms"] for r in k]


def spread_of(ms):
    return f"median {statistics.median(ms):.3f} ms (min {min(ms):.3f}, max {max(ms):.3f})"


def step_floor(a):
    from spnerf_amd import visibility_floor
    from view_bench import stats, timed
    dev = torch.device("cuda", 0)
    _, _, grid, prior, dirs, spread, floor = lidar_floor(dev)
    ms = by_timer(lambda: visibility_floor(prior, grid, dirs), "occlusion_floor", a)
    d = dirs.cpu().numpy()
    finite = torch.isfinite(floor)
    return [f"{torch.cuda.get_device_name(0)}; {a.calls} calls after {a.warmup} warm-up",
            "lines of sight (east, north, up): " + "; ".join(f"({x:+.3f}, {y:+.3f}, {z:.3f})" for x, y, z in d)
            + f"; largest spread {float(spread.max()):.2e}",
            f"  occlusion_floor, 4 views over the {SIDE} x {SIDE} lidar raster, the reduction and the march by the library's timer: {spread_of(ms)}",
            f"    visibility_floor, whole call (allocates, copies the directions to the host): {stats(timed(lambda: visibility_floor(prior, grid, dirs), a.calls, a.warmup))}",
            f"    {100 * float(finite.float().mean()):.1f} % of the floors are finite; median height of the floor above the raster "
            f"{float((floor - prior.float())[finite & torch.isfinite(prior.float())].median()):.2f} m"]


def step_ungated(a):
    from spnerf_amd import _lib, plane_sweep
    images, cams, grid = scene(torch.device("cuda", 0))
    ms = by_timer(lambda: plane_sweep(images, cams, grid, ALT_LO, STEP, PLANES, radius=RADIUS), "sweep", a)
    return [f"  plane_sweep of {os.path.basename(_lib.LIB_PATH)}, the launch by the library's timer:           {spread_of(ms)}"]


def step_gated(a):
    from spnerf_amd import visible_sweep
    dev = torch.device("cuda", 0)
    images, cams, grid = scene(dev)
    floor = torch.full((len(cams), SIDE, SIDE), float("-inf"), device=dev)
    ms = by_timer(lambda: visible_sweep(images, cams, grid, ALT_LO, STEP, PLANES, floor, slack=STEP, radius=RADIUS), "occlusion_sweep", a)
    return [f"  visible_sweep with every floor -inf, the launch by the library's timer:                {spread_of(ms)}"]


def step_real(a):
    from spnerf_amd import plane_sweep, visible_sweep
    dev = torch.device("cuda", 0)
    images, cams, grid, _, _, _, floor = lidar_floor(dev)
    ms = by_timer(lambda: visible_sweep(images, cams, grid, ALT_LO, STEP, PLANES, floor, slack=STEP, radius=RADIUS), "occlusion_sweep", a)
    reach = torch.tensor([ALT_LO + k * STEP + STEP for k in range(PLANES)], dtype=torch.float64, device=dev)
    gated = (reach[:, None, None, None] < floor.double()[None]).float().mean()
    out = visible_sweep(images, cams, grid, ALT_LO, STEP, PLANES, floor, slack=STEP, radius=RADIUS)
    plain = plane_sweep(images, cams, grid, ALT_LO, STEP, PLANES, radius=RADIUS)
    return [f"  visible_sweep with the lidar's floor, slack {STEP} m, the launch by the library's timer: {spread_of(ms)}",
            f"    {100 * float(gated):.1f} % of the (view, cell, plane) triples are gated: not projected, not read; "
            f"{100 * float((out['index'] >= 0).float().mean()):.1f} % of the cells keep a plane ({100 * float((plain['index'] >= 0).float().mean()):.1f} % ungated)"]


def errors(alt, gt):
    alt = alt.cpu().numpy().astype(np.float64)
    ok = np.isfinite(alt) & np.isfinite(gt)
    err = np.abs(alt - gt)[ok]
    return f"{100 * ok.mean():.1f} % of the cells, altitude MAE {float(err.mean()):.3f} m, median |error| {float(np.median(err)):.3f} m"


def step_refine(a):
    from spnerf_amd import plane_sweep, refine_sweep, smooth_sweep
    from view_bench import stats, timed
    dev = torch.device("cuda", 0)
    images, cams, grid = scene(dev)
    gt = lidar()
    prior = torch.tensor(gt, device=dev)
    args, kw = (images, cams, grid, ALT_LO, STEP, PLANES), dict(radius=RADIUS)
    lines = [f"  plane_sweep:                          {errors(plane_sweep(*args, **kw)['altitude'], gt)}",
             f"  smooth_sweep:                         {errors(smooth_sweep(*args, **kw)['altitude'], gt)}; whole call {stats(timed(lambda: smooth_sweep(*args, **kw), a.calls, a.warmup))}"]
    for name, extra in (("refine_sweep (its own first pass)", {}), ("refine_sweep(prior=the lidar raster)", dict(prior=prior))):
        for slack in (STEP, 2.0):
            out = refine_sweep(*args, slack=slack, **kw, **extra)
            ms = timed(lambda: refine_sweep(*args, slack=slack, **kw, **extra), a.calls, a.warmup)
            lines.append(f"  {name}, slack {slack} m: {errors(out['altitude'], gt)}; median raw ZNCC at the pick "
                         f"{float(out['photo'].nanmedian()):.3f}; whole call {stats(ms)}")
    return lines


STEPS = {"floor": step_floor, "ungated": step_ungated, "gated": step_gated, "real": step_real, "refine": step_refine}


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
    order = ["floor"] + ["ungated", "gated"] * a.rounds + ["real", "refine"]
    lines = []
    for step in order:
        env = dict(os.environ)
        if step == "ungated" and a.parent_lib:
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
