"""Time the DSM view on one GPU and say what priors cast from a swept DSM are worth: the workload of
tools/sweep_bench.py — the four shipped JAX_269 cameras over the lidar ROI (256 m square, UTM zone 17) on a
512 x 512 grid of 0.5 m — seen from the cameras between −30 m and 2 m.

Steps, each a fresh process under a time limit of its own; a step is not started when the one before it
fails:

* ``lidar`` / ``base`` — ``view_dsm`` for every pixel of each of the four cameras at downscale 4 over the lidar
  raster of tests/golden/dsm_truth.npz and over ``pyramid_sweep(...)["base"]``: the two launches (the partial
  maxima and the cast) by the library's own timer (HIP events around them, class "dsmview_cast") beside the
  models — 1.5e4 fp64 operations per pixel (two localisations of eight iterations, two forward projections;
  the walk's thirty per step are not counted), and bytes: the DSM once and 33 B written per pixel — then the
  whole call by device events, which adds the allocation of the five planes and the upload of the camera;
* ``full`` — the same for one full-resolution camera at ``stride=4`` over the lidar raster;
* ``quality`` — per camera at full resolution and stride 4: ``view_dsm`` over ``pyramid_sweep``'s ``base`` and over
  the lidar raster, the weight ``sample_at(photo, cell, "nearest")`` of the swept cast (what ``dsm_depth_priors``
  keeps as ``correl``; ``photo`` is the raw ZNCC at the pick), and over the pixels both casts hit, at
  ``min_weight`` None, 0.25 and 0.45: the MAE and the median of |depth − lidar depth| in metres, plain and
  weighted by max(correl, 0), and the same of the altitudes.  Recorded only: there is no threshold;
* ``train`` (with ``--parent-lib NAME``) — ``bench.py --gpus 1 --steps 20 --warmup 5``, the training step, which
  takes none of these paths, with a build of the parent commit beside libspnerf_amd.so and with this tree's
  library, alternated ``--rounds`` times.

    python tools/dsm_view_bench.py [--calls 5] [--warmup 1] [--rounds 3] [--parent-lib NAME] [--out profiles/r25/dsm_view.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from sweep_bench import ALT_LO, FP64_TFLOPS, HBM_GBS, PLANES, RADIUS, SIDE, STEP, VIEWS, scene   # noqa: E402

ALT_HI = ALT_LO + PLANES * STEP
FLOP_PER_PIXEL = 1.5e4
LIMITS = {"lidar": 180, "base": 240, "full": 180, "quality": 300, "train": 300}   # seconds per step
MIN_WEIGHTS = (None, 0.25, 0.45)


def lidar(dev):
    gt = np.load(os.path.join(ROOT, "tests", "golden", "dsm_truth.npz"))["gt"].astype(np.float32)
    assert gt.shape == (SIDE, SIDE)
    return torch.tensor(gt, device=dev)


def swept(dev):
    from spnerf_amd import pyramid_sweep
    images, cams, grid = scene(dev)
    return pyramid_sweep(images, cams, grid, ALT_LO, STEP, PLANES, radius=RADIUS)


def time_cast(dsm, grid, cam, rect, stride, a):
    """One line: the library's timer, the models and the whole call of one cast."""
    from spnerf_amd import _lib, view_dsm
    from view_bench import stats, timed
    call = lambda: view_dsm(dsm, grid, cam, alt_lo=ALT_LO, alt_hi=ALT_HI, rect=rect, stride=stride)   # noqa: E731

    def one():
        _lib.prof_reset()
        call()
        return _lib.prof_read("dsmview_cast")

    for _ in range(a.warmup):
        call()
    _lib.prof_enable(True)
    k = [one() for _ in range(a.calls)]
    _lib.prof_enable(False)
    assert all(r["launches"] == 1 for r in k)
    pixels = rect[2] * rect[3]
    ms, flop, by = statistics.median(r["ms"] for r in k), k[0]["flop"], k[0]["bytes"]
    assert flop == pixels * FLOP_PER_PIXEL and by == 4 * SIDE * SIDE + 33 * pixels
    hits = float((call()["hit"] == 1).float().mean())
    return [f"  {rect[2]} x {rect[3]} pixels, stride {stride}: {100 * hits:.1f} % hit; both launches by the library's timer: median {ms:.4f} ms, "
            f"min {min(r['ms'] for r in k):.4f} ms, max {max(r['ms'] for r in k):.4f} ms",
            f"    fp64 model {flop / 1e9:.2f} GFLOP -> {flop / ms / 1e9:.2f} TFLOPS, {100 * flop / ms / 1e9 / FP64_TFLOPS:.1f} % of the fp64 vector peak; "
            f"byte model {by / 1e6:.2f} MB -> {by / ms / 1e6:.1f} GB/s, {100 * by / ms / 1e6 / HBM_GBS:.2f} % of the HBM peak",
            f"    view_dsm, whole call: {stats(timed(call, a.calls, a.warmup))}"]


def four_cameras(dsm, what, a):
    _, cams, grid = scene(torch.device("cuda", 0))
    lines = [f"view_dsm over {what}, {SIDE} x {SIDE} cells of {grid.resolution} m ({100 * float(torch.isfinite(dsm).float().mean()):.1f} % finite), altitudes "
             f"{ALT_LO} m to {ALT_HI} m, every pixel of the four shipped cameras at downscale 4:"]
    for cam in cams:
        lines += time_cast(dsm, grid, cam, (0, 0, cam.shape[1], cam.shape[0]), 1, a)
    return lines


def step_lidar(a):
    dev = torch.device("cuda", 0)
    head = [f"{torch.cuda.get_device_name(0)}; {a.calls} calls after {a.warmup} warm-up; peaks taken as {HBM_GBS:.0f} GB/s of HBM and {FP64_TFLOPS} TFLOPS "
            "of vector fp64; what bounds the kernel has not been measured: the models only say how far either peak is"]
    return head + four_cameras(lidar(dev), "the lidar raster", a)


def step_base(a):
    return four_cameras(swept(torch.device("cuda", 0))["base"], 'pyramid_sweep(...)["base"]', a)


def full_cameras():
    from spnerf_amd import rectify
    from spnerf_amd.satellite import load_cameras
    metas = load_cameras()["images"]
    return [rectify.Camera.from_meta(metas[v], 1) for v in VIEWS]


def quarter(cam):
    return (0, 0, (cam.shape[1] - 1) // 4 + 1, (cam.shape[0] - 1) // 4 + 1)


def step_full(a):
    dev = torch.device("cuda", 0)
    _, _, grid = scene(dev)
    cam = full_cameras()[0]
    return [f"view_dsm over the lidar raster, camera {VIEWS[0]} at full resolution ({cam.shape[0]} x {cam.shape[1]}), stride 4:"] + \
        time_cast(lidar(dev), grid, cam, quarter(cam), 4, a)


def weighted_median(x, w):
    order = np.argsort(x)
    c = np.cumsum(w[order])
    return float(x[order][np.searchsorted(c, 0.5 * c[-1])])


def step_quality(a):
    from spnerf_amd import sample_at, view_dsm
    dev = torch.device("cuda", 0)
    _, _, grid = scene(dev)
    out, gt = swept(dev), lidar(dev)
    base, photo = out["base"], out["photo"]
    err = (base - gt).abs()[torch.isfinite(base)]
    lines = [f'priors cast from pyramid_sweep(...)["base"] against priors cast from the lidar raster, full-resolution cameras at stride 4; on the grid the '
             f"base has MAE {float(err.mean()):.3f} m, median |error| {float(err.median()):.3f} m against the lidar, median raw ZNCC at the pick "
             f"{float(photo.nanmedian()):.3f}",
             "  camera, min_weight: share of the pixels both casts hit; |depth − lidar depth| MAE / median, weighted by correl MAE / median; "
             "|altitude − lidar altitude| MAE / median, weighted MAE / median (metres)"]
    for v, cam in zip(VIEWS, full_cameras()):
        kw = dict(alt_lo=ALT_LO, alt_hi=ALT_HI, rect=quarter(cam), stride=4)
        s, t = view_dsm(base, grid, cam, **kw), view_dsm(gt, grid, cam, **kw)
        correl = sample_at(photo, s["cell"], "nearest").cpu().numpy().astype(np.float64)
        both = ((s["hit"] == 1) & (t["hit"] == 1)).cpu().numpy() & np.isfinite(correl)
        dd = np.abs(s["depth"].cpu().numpy().astype(np.float64) - t["depth"].cpu().numpy())
        da = np.abs(s["altitude"].cpu().numpy().astype(np.float64) - t["altitude"].cpu().numpy())
        for mw in MIN_WEIGHTS:
            keep = both & ((correl >= mw) if mw is not None else True)
            w = np.maximum(correl[keep], 0.0)
            cells = []
            for d in (dd[keep], da[keep]):
                cells.append(f"{d.mean():.3f} / {np.median(d):.3f}, weighted {float((w * d).sum() / w.sum()):.3f} / {weighted_median(d, w):.3f}")
            lines.append(f"  {v}, min_weight {mw}: {100 * keep.mean():.1f} %; depth {cells[0]}; altitude {cells[1]}")
    return lines


def step_train(a):
    from spnerf_amd import _lib
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], stdout=subprocess.PIPE,
                       text=True, check=True)
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    return [f"  bench.py --gpus 1 --steps 20 --warmup 5 ({os.path.basename(_lib.LIB_PATH)}): {line['ms_per_step']:.3f} ms per step, "
            f"{line['value'] / 1e6:.3f} M {line['unit']}"]


STEPS = {"lidar": step_lidar, "base": step_base, "full": step_full, "quality": step_quality, "train": step_train}


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
    order = [("lidar", None), ("base", None), ("full", None), ("quality", None)]
    if a.parent_lib:
        order += [("train", a.parent_lib), ("train", None)] * a.rounds
    lines = []
    for step, library in order:
        env = dict(os.environ)
        if library:
            env["SPNERF_AMD_LIB"] = library
        if step == "train" and not any(ln.startswith("the training step") for ln in lines):
            lines.append(f"the training step, the parent commit's library ({a.parent_lib}) alternated with this tree's, {a.rounds} rounds:")
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
