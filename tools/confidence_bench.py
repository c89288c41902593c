"""Time the confidence launch on one GPU and say how good each of its planes is as a confidence: the workload of
tools/sweep_bench.py — the four shipped JAX_269 cameras over the lidar ROI (256 m square, UTM zone 17) on a
512 x 512 grid of 0.5 m, 64 planes of 0.5 m from −30 m, window radius 2 — against the lidar raster
(tests/golden/dsm_truth.npz).

Steps, each a fresh process under a time limit of its own; a step is not started when the one before it fails:

* ``time`` — ``conf_volume`` by the library's own timer (HIP events around the launch) on ``smooth_sweep``'s
  aggregated volume (64 x 512 x 512) and on a 4 x 4 tiling of it (64 x 2048 x 2048), with all nine outputs and with
  ``index`` + ``margin`` only, beside its byte model — one read of the volume plus the planes written — as a share of
  the HBM peak, and beside ``sgm_pick`` timed in the same process; the time per byte of each.  What bounds the
  kernel is not measured;
* ``quality`` — on ``smooth_sweep``'s altitude: the sparsification area and the MAE of the best 50 % and 75 % of the
  cells ranked by ``photo``, ``score``, ``margin``, ``peak_margin``, ``curvature``, −``support``, −``peaks``, ``mlm``
  and −``spread``, from the raw and from the aggregated volume, over tau 0.02, 0.05, 0.1 and temperature 0.02, 0.05,
  0.1, 0.2, with the oracle's area and a flat curve's beside them.  So that every ranking is over the same cells, a
  ``margin`` or ``peak_margin`` that is NaN (no rival) ranks above every cell that has one, and a ``curvature`` that
  is NaN (the pick at the volume's edge or beside an unscored plane) below every cell that has one;
* ``clean`` — for the best-ranked of the planes ``bootstrap_sweep`` takes, on the aggregated volume: ``clean_dsm`` with
  a fill, and ``bootstrap_sweep(weight=…)``, with ``min_weight`` set so that the share of the cells ``photo >= 0.25``
  rejects is rejected, beside the ``photo`` rows;
* ``train`` (with ``--parent-lib NAME``) — ``bench.py --gpus 1 --steps 20 --warmup 5``, the training step, which takes
  none of these paths, with a build of the parent commit beside libspnerf_amd.so and with this tree's library,
  alternated ``--rounds`` times.

    python tools/confidence_bench.py [--calls 5] [--warmup 1] [--rounds 3] [--parent-lib NAME] [--only time,quality,clean,train]
                                     [--out profiles/r27/confidence.txt] [--bench-out FILE: the training step's lines apart]
"""
import argparse
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from clean_bench import by_timer, errors, lidar   # noqa: E402
from dsm_view_bench import step_train   # noqa: E402
from sweep_bench import ALT_LO, HBM_GBS, PLANES, RADIUS, STEP, scene   # noqa: E402

LIMITS = {"time": 240, "quality": 420, "clean": 300, "train": 300}   # seconds per step
TAUS, TEMPERATURES = (0.02, 0.05, 0.1), (0.02, 0.05, 0.1, 0.2)
GATES = ("margin", "peak_margin", "curvature", "mlm")                 # the planes bootstrap_sweep(weight=) takes
REACH = 16


def per_byte(name, ms, model, note=""):
    med = statistics.median(ms)
    return (f"    {name}: median {med:.4f} ms (min {min(ms):.4f}, max {max(ms):.4f}); byte model {model / 1e6:.2f} MB -> {model / med / 1e6:.1f} GB/s, "
            f"{100 * model / med / 1e6 / HBM_GBS:.2f} % of the HBM peak; {1e9 * med / model:.4f} ps per byte{note}")


def step_time(a):
    from spnerf_amd import sgm, smooth_sweep, volume_confidence
    dev = torch.device("cuda", 0)
    images, cams, grid = scene(dev)
    first = smooth_sweep(images, cams, grid, ALT_LO, STEP, PLANES, radius=RADIUS, volume=True)
    lines = [f"{torch.cuda.get_device_name(0)}; {a.calls} calls after {a.warmup} warm-up; the peak taken as {HBM_GBS:.0f} GB/s of HBM; what bounds the kernel "
             "has not been measured: the byte models only say how far the peak is"]
    for tiles in (1, 4):
        agg, raw = (first[k].repeat(1, tiles, tiles).contiguous() for k in ("aggregated", "volume"))
        K, H, W = agg.shape
        lines.append(f"smooth_sweep's aggregated volume{'' if tiles == 1 else ', tiled 4 x 4'}: {K} x {H} x {W}, {100 * float(torch.isnan(agg).float().mean()):.2f} % NaN; "
                     f"{K * H * W / 1e6:.1f} M fp64 exp per launch that writes mlm or spread")
        rows = {}
        for what, planes in (("all nine outputs", None), ("index + margin (a second pass, no exp)", ("index", "margin")), ("index alone (no second pass)", ("index",))):
            ms, model = by_timer(lambda: volume_confidence(agg, ALT_LO, STEP, planes=planes), ("conf_volume",), a)
            rows[what] = statistics.median(ms["conf_volume"]) / model["conf_volume"]
            lines.append(per_byte(f"conf_volume, {what}", ms["conf_volume"], model["conf_volume"]))
        ms, model = by_timer(lambda: sgm.pick(agg, raw, ALT_LO, STEP), ("sgm_pick",), a)
        pick = statistics.median(ms["sgm_pick"]) / model["sgm_pick"]
        two = 2.0 * K * H * W * 4 + 16.0 * H * W
        lines.append(per_byte("sgm_pick", ms["sgm_pick"], model["sgm_pick"], f" (the library's model: one read of the aggregated volume, one raw entry per cell, four planes written; "
                              f"as two reads of the volume, {two / 1e6:.2f} MB: {1e9 * statistics.median(ms['sgm_pick']) / two:.4f} ps per byte)"))
        for what, r in rows.items():
            lines.append(f"    conf_volume, {what}: {r / pick:.2f} x sgm_pick's time per byte")
    return lines


def ranked(conf, name):
    """The plane as a ranking over every cell with a pick: see the module's note on NaN."""
    plane = conf[name].double()
    if name in ("margin", "peak_margin"):
        return torch.where(torch.isnan(plane) & (conf["index"] >= 0), torch.full_like(plane, 4.0), plane)   # scores lie in [−1, 1]: no margin reaches 4
    if name == "curvature":
        return torch.where(torch.isnan(plane) & (conf["index"] >= 0), torch.full_like(plane, -1.0), plane)
    return plane


def row_of(name, err, conf):
    from spnerf_amd import sparsification
    s = sparsification(err, conf, steps=100)
    return s["area"], f"      {name:<28s} area {s['area']:.4f}; MAE of the best 50 % {float(s['curve'][50]):.3f} m, of the best 75 % {float(s['curve'][25]):.3f} m; {s['cells']} cells"


def abs_error(alt, gt, dev):
    err = (alt.double() - torch.tensor(gt, device=dev)).abs()
    return torch.where(torch.isfinite(err), err, torch.full_like(err, float("nan")))


def step_quality(a):
    from spnerf_amd import smooth_sweep, sparsification, volume_confidence
    dev = torch.device("cuda", 0)
    images, cams, grid = scene(dev)
    first = smooth_sweep(images, cams, grid, ALT_LO, STEP, PLANES, radius=RADIUS, volume=True)
    err = abs_error(first["altitude"], lidar(), dev)
    oracle = sparsification(err, -err, steps=100)
    lines = ["smooth_sweep's altitude against the lidar raster: %.1f %% of the cells compared, MAE %.3f m, median |error| %.3f m" % errors(first["altitude"], lidar()),
             f"sparsification over the removed shares 0 .. 0.99 (100 steps): area of the oracle (confidence = −error) {oracle['area']:.4f}, of a flat curve (a confidence "
             f"that says nothing) 0.9900; MAE of the oracle's best 50 % {float(oracle['curve'][50]):.3f} m, best 75 % {float(oracle['curve'][25]):.3f} m",
             "  the height of the peak, as the picks give it:"]
    for name in ("photo", "score"):
        lines.append(row_of(name, err, first[name])[1])
    best = {}
    for what, volume in (("raw", first["volume"]), ("aggregated", first["aggregated"])):
        lines.append(f"  from the {what} volume (exclude 1):")
        conf = volume_confidence(volume, ALT_LO, STEP)
        rows = [(name,) + row_of(name, err, ranked(conf, name)) for name in ("margin", "peak_margin", "curvature")]
        for tau in TAUS:
            conf = volume_confidence(volume, ALT_LO, STEP, tau=tau, planes=("support", "peaks"))
            rows += [(f"-{name}, tau {tau}",) + row_of(f"-{name}, tau {tau}", err, -conf[name].double()) for name in ("support", "peaks")]
        for temperature in TEMPERATURES:
            conf = volume_confidence(volume, ALT_LO, STEP, temperature=temperature, planes=("mlm", "spread"))
            rows += [(f"mlm, temperature {temperature}",) + row_of(f"mlm, temperature {temperature}", err, conf["mlm"]),
                     (f"-spread, temperature {temperature}",) + row_of(f"-spread, temperature {temperature}", err, -conf["spread"].double())]
        lines += [r[2] for r in rows]
        best[what] = min(rows, key=lambda r: r[1])
        lines.append(f"    the lowest area from the {what} volume: {best[what][0]}, {best[what][1]:.4f}")
        for kind, pick in (("tau", ("-support", "-peaks")), ("temperature", ("mlm", "-spread"))):
            low = min((r for r in rows if r[0].split(",")[0] in pick), key=lambda r: r[1])
            lines.append(f"    the lowest area among the rows that take a {kind}: {low[0]}, {low[1]:.4f}")
    return lines


def gate_for_share(weight, finite, share):
    """min_weight at which ``share`` of the cells — counted as clean_dsm counts them: finite altitude, weight below or
    NaN — is rejected, and the share it rejects."""
    w = weight[finite]
    lost = int(torch.isnan(w).sum())
    ordered = torch.sort(w[~torch.isnan(w)]).values
    want = min(max(int(round(share * weight.numel())) - lost, 0), ordered.numel() - 1)
    level = float(ordered[want])
    return level, float((finite & ~(weight >= level)).float().mean())


def step_clean(a):
    from spnerf_amd import bootstrap_sweep, clean, clean_dsm, smooth_sweep, volume_confidence
    dev = torch.device("cuda", 0)
    images, cams, grid = scene(dev)
    gt = lidar()
    args = (images, cams, grid, ALT_LO, STEP, PLANES)
    first = smooth_sweep(*args, radius=RADIUS, volume=True)
    err = abs_error(first["altitude"], gt, dev)
    conf = volume_confidence(first["aggregated"], ALT_LO, STEP)
    areas = {name: row_of(name, err, ranked(conf, name))[0] for name in GATES}
    name = min(areas, key=areas.get)
    finite = torch.isfinite(first["altitude"])
    share = float((finite & ~(first["photo"] >= clean.MIN_WEIGHT)).float().mean())
    level, got = gate_for_share(conf[name], finite, share)
    kw = dict(max_diff=clean.MAX_DIFF_STEPS * STEP, max_size=clean.SPECKLE_CELLS, radius=clean.MEDIAN_RADIUS)
    lines = [f"the planes bootstrap_sweep takes, by sparsification area on the aggregated volume at the defaults: " + ", ".join(f"{k} {v:.4f}" for k, v in areas.items())
             + f"; the best-ranked: {name}",
             f"photo >= {clean.MIN_WEIGHT} rejects {100 * share:.2f} % of the cells; {name} >= {level!r} rejects {100 * got:.2f} % (a NaN is rejected, as clean_dsm does)",
             "altitude against the lidar raster: share of the cells compared, MAE, median |error| (metres); lower is better, and the MAEs are bit-reproducible",
             "  smooth_sweep:                                              %.1f %%, %.3f, %.3f" % errors(first["altitude"], gt)]
    for what, weight, min_weight in (("photo", first["photo"], clean.MIN_WEIGHT), (name, conf[name], level)):
        out = clean_dsm(first["altitude"], weight=weight, min_weight=min_weight, reach=REACH, **kw)
        lines.append(f"  clean_dsm(weight={what}) with a fill of reach {REACH}:".ljust(61) + "%.1f %%, %.3f, %.3f" % errors(out["dsm"], gt)
                     + f"; rejected by the weight {100 * float((out['rejected'] & 1 != 0).float().mean()):.2f} %, filled {100 * float((out['filled'] != 0).float().mean()):.2f} %")
    maes = {}
    for what, min_weight in (("photo", clean.MIN_WEIGHT), (name, level)):
        out = bootstrap_sweep(*args, sweep_radius=RADIUS, weight=what, min_weight=min_weight)
        cells, maes[what], med = errors(out["altitude"], gt)
        lines.append(f"  bootstrap_sweep(weight={what!r}, min_weight={min_weight!r}):".ljust(61) + f"{cells:.1f} %, {maes[what]:.3f}, {med:.3f}")
    lines.append(f"  the parent's bootstrap_sweep: 7.57 m (profiles/r26/clean.txt).  {name} {'lowers' if maes[name] < maes['photo'] else 'does not lower'} the two-pass MAE: "
                 f"{maes[name] - maes['photo']:+.3f} m against photo.  No default moves: bootstrap_sweep's weight stays 'photo'")
    return lines


STEPS = {"time": step_time, "quality": step_quality, "clean": step_clean, "train": step_train}


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
    order = [(s, None) for s in ("time", "quality", "clean") if s in only]
    if a.parent_lib and "train" in only:
        order += [("train", a.parent_lib), ("train", None)] * a.rounds
    lines, bench = [], []                                                 # the confidence's own steps; the training step
    for step, library in order:
        env = dict(os.environ)
        if library:
            env["SPNERF_AMD_LIB"] = library
        if step == "train" and not bench:
            bench.append(f"the training step, the parent commit's library ({a.parent_lib}) alternated with this tree's, {a.rounds} rounds:")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--calls", str(a.calls), "--warmup", str(a.warmup)],
                           stdout=subprocess.PIPE, text=True, timeout=LIMITS[step], env=env)
        if step == "train" and len(bench) == 1:
            print(bench[0])
        (bench if step == "train" else lines).extend(r.stdout.splitlines())
        print(r.stdout, end="", flush=True)                               # each step's lines as the step ends
        if r.returncode != 0:
            sys.exit(f"step {step} ended with status {r.returncode}: nothing further is started")
    for path, text in ((a.out, lines if a.bench_out else lines + bench), (a.bench_out, bench)):
        if path and text:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
