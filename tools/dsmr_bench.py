"""Time the DSM registration on the full 512 x 512 lidar truth pair (tests/golden/dsm_truth.npz):
``compute_shift`` followed by the fused shift-and-MAE on the GPU (median of the calls after
warm-up, device events around both), and the numpy restatement (tests/dsmr_numpy.py) once on the
CPU.  The pair: the truth, and the truth rolled by (3, -2) cells with an offset, noise and holes.

    python tools/dsmr_bench.py [--calls 30] [--warmup 5] [--out profiles/r09/dsmr.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.calls < 20:
        ap.error("--calls: at least 20")
    from spnerf_amd import _eval_lib, dsm
    import dsmr_numpy as dn

    gt = np.load(os.path.join(ROOT, "tests", "golden", "dsm_truth.npz"))["gt"].astype(np.float64)
    rng = np.random.default_rng(0)
    pred = np.roll(gt, (-2, 3), axis=(0, 1)) + 1.5 + 0.05 * rng.standard_normal(gt.shape)
    pred[rng.random(gt.shape) < 0.1] = np.nan
    dev = torch.device("cuda", 0)
    u, v = torch.tensor(gt, device=dev), torch.tensor(pred, device=dev)
    sums = torch.empty(_eval_lib.DSM_SUMS_DOUBLES, dtype=torch.float64, device=dev)

    def call():
        reg = dsm._register(u, v, 5, (0, 0))
        dsm._apply(v, reg=reg.device_result, ref=u, sums=sums)
        return reg

    for _ in range(args.warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        reg = call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    total, count = sums[:2].cpu().tolist()
    t0 = time.perf_counter()
    dx, dy, _, bb, m = dn.compute_shift(gt, pred, scaling=False)
    err = dn.apply_shift(pred, dx, dy, 1.0, bb) - gt
    mae = float(np.nanmean(np.abs(err)))
    cpu_s = time.perf_counter() - t0
    lines = [
        f"DSM registration, 512 x 512 pair, irange 5, {dsm.pyramid_levels(512, 512)} levels",
        f"GPU ({torch.cuda.get_device_name(0)}): compute_shift + fused MAE, device events, {args.calls} calls after "
        f"{args.warmup} warm-up: median {statistics.median(ms):.3f} ms, min {min(ms):.3f} ms, max {max(ms):.3f} ms",
        f"CPU numpy restatement, once: {cpu_s * 1e3:.1f} ms",
        f"shift GPU ({reg.dx}, {reg.dy}) / numpy ({dx}, {dy}); MAE GPU {total / count:.9f} / numpy {mae:.9f}",
    ]
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
