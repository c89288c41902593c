"""Time the DSM cleaning on one GPU and say what a cleaned prior does to the two-pass sweep: the workload of
tools/sweep_bench.py — the four shipped JAX_269 cameras over the lidar ROI (256 m square, UTM zone 17) on a
512 x 512 grid of 0.5 m, 64 planes of 0.5 m from −30 m, window radius 2.

Steps, each a fresh process under a time limit of its own; a step is not started when the one before it
fails:

* ``time`` — on ``smooth_sweep``'s altitude (512 x 512) and on a 4 x 4 tiling of it (2048 x 2048): the four
  launches of ``speckle_filter`` each by the library's own timer (HIP events around the launch, classes
  "clean_local", "clean_merge", "clean_flatten", "clean_apply"), ``median_dsm`` at radius 1, 2, 3 ("clean_median")
  and ``fill_holes`` at reach 16 ("clean_fill"), each beside its byte model — 4 B read and 4 B written per cell for
  the median, 4 + 4 + 1 for the fill, for the speckle filter the sum of its passes: 8 B per cell in the local
  pass, 16 B per pair of cells across a tile border, 12 B in the flatten, 20 B in the apply — as a share of the
  HBM peak; then the whole calls by device events.  What bounds each kernel is not measured;
* ``quality`` — altitude MAE and median |error| against the lidar raster (tests/golden/dsm_truth.npz) of
  ``smooth_sweep``, of ``refine_sweep`` from its own first pass, and of the two-pass sweep over a cleaned first
  pass for ``max_size`` 25, 100, 400, 1600 cells x ``max_diff`` 1, 2 steps x median radius 0, 1, 2 x
  ``min_weight`` None, 0.25, with the share of the cells each stage rejects.  The first pass is computed once and
  every row is ``clean_dsm`` → ``refine_sweep(prior=cleaned)``, the chain ``bootstrap_sweep`` is (tests/test_gpu_clean.py
  holds it to those bytes); the best row is run through ``bootstrap_sweep`` itself as a check;
* ``pyramid`` — ``clean_dsm`` with a fill over ``pyramid_sweep``'s altitude: MAE and the share of NaN cells before
  and after;
* ``train`` (with ``--parent-lib NAME``) — ``bench.py --gpus 1 --steps 20 --warmup 5``, the training step, which
  takes none of these paths, with a build of the parent commit beside libspnerf_amd.so and with this tree's
  library, alternated ``--rounds`` times.

    python tools/clean_bench.py [--calls 5] [--warmup 1] [--rounds 3] [--parent-lib NAME] [--only time,quality,pyramid,train]
                                [--out profiles/r26/clean.txt] [--bench-out profiles/r26/bench.txt]
"""
import argparse
import itertools
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from dsm_view_bench import step_train   # noqa: E402
from sweep_bench import ALT_LO, HBM_GBS, PLANES, RADIUS, SIDE, STEP, scene   # noqa: E402

LIMITS = {"time": 240, "quality": 420, "pyramid": 240, "train": 300}   # seconds per step
SPECKLE_CLASSES = ("clean_local", "clean_merge", "clean_flatten", "clean_apply")
MAX_SIZES, MAX_DIFFS, RADII, MIN_WEIGHTS = (25, 100, 400, 1600), (1, 2), (0, 1, 2), (None, 0.25)


def lidar():
    gt = np.load(os.path.join(ROOT, "tests", "golden", "dsm_truth.npz"))["gt"].astype(np.float64)
    assert gt.shape == (SIDE, SIDE)
    return gt


def errors(alt, gt):
    alt = alt.cpu().numpy().astype(np.float64)
    ok = np.isfinite(alt) & np.isfinite(gt)
    err = np.abs(alt - gt)[ok]
    return 100 * ok.mean(), float(err.mean()), float(np.median(err))


def by_timer(call, classes, a):
    """{class: [ms per call]} and {class: model bytes} of one call's launches by the library's timer."""
    from spnerf_amd import _lib
    for _ in range(a.warmup):
        call()
    _lib.prof_enable(True)
    ms, model = {c: [] for c in classes}, {}
    for _ in range(a.calls):
        _lib.prof_reset()
        call()
        for c in classes:
            r = _lib.prof_read(c)
            assert r["launches"] == 1, (c, r)
            ms[c].append(r["ms"])
            model[c] = r["bytes"]
    _lib.prof_enable(False)
    return ms, model


def line_of(name, ms, model):
    med = statistics.median(ms)
    return (f"    {name}: median {med:.4f} ms (min {min(ms):.4f}, max {max(ms):.4f}); byte model {model / 1e6:.2f} MB -> {model / med / 1e6:.1f} GB/s, "
            f"{100 * model / med / 1e6 / HBM_GBS:.2f} % of the HBM peak")


def step_time(a):
    from spnerf_amd import fill_holes, median_dsm, smooth_sweep, speckle_filter
    from view_bench import stats, timed
    dev = torch.device("cuda", 0)
    images, cams, grid = scene(dev)
    roi = smooth_sweep(images, cams, grid, ALT_LO, STEP, PLANES, radius=RADIUS)["altitude"]
    lines = [f"{torch.cuda.get_device_name(0)}; {a.calls} calls after {a.warmup} warm-up; the peak taken as {HBM_GBS:.0f} GB/s of HBM; what bounds each kernel "
             "has not been measured: the byte models only say how far the peak is"]
    for what, dsm in (("smooth_sweep's altitude", roi), ("a 4 x 4 tiling of it", roi.repeat(4, 4).contiguous())):
        H, W = dsm.shape
        out = speckle_filter(dsm, max_diff=STEP, max_size=100)
        holes = 100 * float((~torch.isfinite(dsm)).float().mean())
        lines.append(f"{what}, {H} x {W} cells, {holes:.2f} % holes; max_diff {STEP} m: {int(torch.unique(out['label']).numel() - (1 if holes else 0))} components, "
                     f"the largest of {int(out['size'].max())} cells, {100 * float(((out['size'] >= 1) & (out['size'] <= 100)).float().mean()):.2f} % of the cells in "
                     "components of at most 100")
        ms, model = by_timer(lambda: speckle_filter(dsm, max_diff=STEP, max_size=100), SPECKLE_CLASSES, a)
        for c in SPECKLE_CLASSES:
            lines.append(line_of(c, ms[c], model[c]))
        total = [sum(ms[c][k] for c in SPECKLE_CLASSES) for k in range(a.calls)]
        lines.append(line_of("the four launches", total, sum(model.values())))
        lines.append(f"    speckle_filter, whole call (allocates, clears the counts, waits for the bound's word): {stats(timed(lambda: speckle_filter(dsm, max_diff=STEP, max_size=100), a.calls, a.warmup))}")
        for r in (1, 2, 3):
            ms, model = by_timer(lambda: median_dsm(dsm, radius=r), ("clean_median",), a)
            lines.append(line_of(f"clean_median, radius {r}", ms["clean_median"], model["clean_median"]))
        lines.append(f"    median_dsm(radius=1), whole call: {stats(timed(lambda: median_dsm(dsm, radius=1), a.calls, a.warmup))}")
        holed = out["dsm"]
        ms, model = by_timer(lambda: fill_holes(holed, reach=16), ("clean_fill",), a)
        lines.append(line_of(f"clean_fill, reach 16, over the speckle filter's output ({100 * float((~torch.isfinite(holed)).float().mean()):.2f} % holes)", ms["clean_fill"],
                             model["clean_fill"]))
        lines.append(f"    fill_holes(reach=16), whole call: {stats(timed(lambda: fill_holes(holed, reach=16), a.calls, a.warmup))}")
    return lines


def share(mask):
    return 100 * float(mask.float().mean())


def step_quality(a):
    from spnerf_amd import bootstrap_sweep, clean_dsm, refine_sweep, smooth_sweep
    dev = torch.device("cuda", 0)
    images, cams, grid = scene(dev)
    gt = lidar()
    args, kw = (images, cams, grid, ALT_LO, STEP, PLANES), dict(radius=RADIUS)
    first = smooth_sweep(*args, **kw)
    lines = ["altitude against the lidar raster: share of the cells compared, MAE, median |error| (metres)",
             "  smooth_sweep:                        %.1f %%, %.3f, %.3f" % errors(first["altitude"], gt),
             "  refine_sweep (its own first pass):   %.1f %%, %.3f, %.3f" % errors(refine_sweep(*args, **kw)["altitude"], gt),
             "  the two-pass sweep over clean_dsm(first pass), reach None; rejected by weight / speckle / changed by the median, % of the cells:"]
    rows = []
    for max_size, steps, radius, mw in itertools.product(MAX_SIZES, MAX_DIFFS, RADII, MIN_WEIGHTS):
        cleaned = clean_dsm(first["altitude"], weight=None if mw is None else first["photo"], min_weight=mw, max_diff=steps * STEP, max_size=max_size,
                            radius=radius)
        out = refine_sweep(*args, prior=cleaned["dsm"], **kw)
        rej = cleaned["rejected"]
        cells, mae, med = errors(out["altitude"], gt)
        rows.append((mae, med, max_size, steps, radius, mw))
        lines.append(f"    max_size {max_size:4d}, max_diff {steps} step, radius {radius}, min_weight {mw}: {cells:.1f} %, {mae:.3f}, {med:.3f}; "
                     f"{share(rej & 1 != 0):.2f} / {share(rej & 2 != 0):.2f} / {share(rej & 4 != 0):.2f}; the prior {share(~torch.isfinite(cleaned['dsm'])):.2f} % holes")
    mae, med, max_size, steps, radius, mw = min(rows)
    out = bootstrap_sweep(*args, max_diff=steps * STEP, max_size=max_size, radius=radius, min_weight=mw, sweep_radius=RADIUS)
    lines.append(f"  the row of the lowest MAE: max_size {max_size}, max_diff {steps} step, radius {radius}, min_weight {mw}: {mae:.3f}, {med:.3f}; "
                 "bootstrap_sweep with these arguments: %.1f %%, %.3f, %.3f" % errors(out["altitude"], gt))
    from spnerf_amd import clean
    out = bootstrap_sweep(*args, sweep_radius=RADIUS)
    lines.append(f"  bootstrap_sweep with its defaults (max_diff {clean.MAX_DIFF_STEPS} steps, max_size {clean.SPECKLE_CELLS}, radius {clean.MEDIAN_RADIUS}, "
                 f"min_weight {clean.MIN_WEIGHT}, no fill): " + "%.1f %%, %.3f, %.3f" % errors(out["altitude"], gt))
    return lines


def step_pyramid(a):
    from spnerf_amd import clean_dsm, pyramid_sweep
    dev = torch.device("cuda", 0)
    images, cams, grid = scene(dev)
    gt = lidar()
    alt = pyramid_sweep(images, cams, grid, ALT_LO, STEP, PLANES, radius=RADIUS)["altitude"]
    lines = ["clean_dsm with a fill over pyramid_sweep's altitude: share of NaN cells, then share compared, MAE, median |error| (metres)",
             f"  before: {share(~torch.isfinite(alt)):.2f} % NaN; " + "%.1f %%, %.3f, %.3f" % errors(alt, gt)]
    for max_size, radius, reach, mode in ((100, 1, 16, "lowest"), (100, 1, 16, "nearest"), (400, 1, 64, "lowest"), (400, 2, 64, "nearest")):
        out = clean_dsm(alt, max_diff=STEP, max_size=max_size, radius=radius, reach=reach, mode=mode)
        rej = out["rejected"]
        lines.append(f"  max_diff {STEP} m, max_size {max_size}, radius {radius}, reach {reach}, {mode}: {share(~torch.isfinite(out['dsm'])):.2f} % NaN; "
                     + "%.1f %%, %.3f, %.3f" % errors(out["dsm"], gt) + f"; rejected by speckle {share(rej & 2 != 0):.2f} %, changed by the median "
                     f"{share(rej & 4 != 0):.2f} %, filled {share(out['filled'] != 0):.2f} %")
    return lines


STEPS = {"time": step_time, "quality": step_quality, "pyramid": step_pyramid, "train": step_train}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench-out", default=None)
    ap.add_argument("--step", choices=["all"] + list(STEPS), default="all")
    ap.add_argument("--only", default=None, help="comma-separated steps of the whole run (default: all of them)")
    a = ap.parse_args()
    if a.step != "all":
        print("\n".join(STEPS[a.step](a)))
        return
    only = list(STEPS) if a.only is None else a.only.split(",")
    unknown = [s for s in only if s not in STEPS]
    if unknown:
        ap.error(f"--only: unknown step(s) {', '.join(map(repr, unknown))}; the steps are {', '.join(STEPS)}")
    if "train" in only and a.only is not None and not a.parent_lib:
        ap.error("--only train needs --parent-lib")
    order = [(s, None) for s in ("time", "quality", "pyramid") if s in only]
    if a.parent_lib and "train" in only:
        order += [("train", a.parent_lib), ("train", None)] * a.rounds
    lines, bench = [], []                                                 # the cleaning's own steps; the training step
    for step, library in order:
        env = dict(os.environ)
        if library:
            env["SPNERF_AMD_LIB"] = library
        if step == "train" and not bench:
            bench.append(f"the training step, the parent commit's library ({a.parent_lib}) alternated with this tree's, {a.rounds} rounds:")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--calls", str(a.calls), "--warmup", str(a.warmup)],
                           stdout=subprocess.PIPE, text=True, timeout=LIMITS[step], env=env)
        (bench if step == "train" else lines).extend(r.stdout.splitlines())
        if r.returncode != 0:
            print("\n".join(lines + bench))
            sys.exit(f"step {step} ended with status {r.returncode}: nothing further is started")
    print("\n".join(lines + bench))
    for path, text in ((a.out, lines), (a.bench_out, bench)):
        if path and text:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
