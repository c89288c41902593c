"""Time one training step two ways on one GPU, in one process, the two alternating, on the bench's
C4 workload (W = 512, bf16 MLP, 64 + 64 guided samples, solar pass, depth + semantic heads) at 4 096
and at 512 rays per step:

  (A) the step as ``bench.TrainStep`` runs it: the batch's indices copied into the static buffer, one
      replay of the render + loss + backward graph, then the library Adam outside the graph on the
      host's scalars (noise_std 0);
  (B) ``spnerf_amd.train.Trainer.step()``: one replay of a graph that also holds the schedule, the
      batch pick and Adam, with every per-step scalar on the device.

Each step is timed with device events around the host call (the step's launches and its device work,
synchronized after every step); the median of the steps after warm-up with the range.  A second
figure per arm: the wall time per step of blocks of steps issued back to back without a sync between
them (what a training loop sees), blocks alternating between the arms.

    python tools/train_bench.py [--steps 30] [--warmup 5] [--out profiles/r16/train_step.txt]
"""
import argparse
import os
import statistics
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return f"median {statistics.median(ms):.3f} ms, min {min(ms):.3f} ms, max {max(ms):.3f} ms"


def block_ms(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def run_size(rays, steps, warmup, say):
    import bench
    import spnerf_amd
    from spnerf_amd.train import Trainer
    dev = torch.device("cuda", 0)
    a = bench.parse_args(["--config", "c4", "--no-cpu-baseline", "--no-secondary", "--global-batch", str(rays)])
    ts = bench.TrainStep(a, "c4", 0, 1, dev)
    if not ts.capture(max(2, warmup)):
        raise SystemExit("train_bench: the bench step's graph capture failed")
    c = ts.c
    torch.manual_seed(0)
    model = spnerf_amd.SPNeRF(num_sem_classes=3, s_embedding_factor=1, layers=8, feat=512, mapping=True, sem=c["sem"],
                              precision=c["precision"]).to(dev)
    targs = types.SimpleNamespace(**vars(ts.args), lr=5e-4, batch_size=rays, max_train_steps=10 ** 9, depth=c["depth"],
                                  ds_lambda=1.0, ds_drop=1, GNLL=False, usealldepth=False, sem=c["sem"], ss_lambda=1.0,
                                  ss_drop=1, first_beta_epoch=2)
    targs.noise_std = 0.0
    tr = Trainer({"coarse": model}, targs, ts.R, seed=0)
    for _ in range(max(3, warmup)):     # the eager first step, the capture, replays
        tr.step()
    torch.cuda.synchronize()
    assert tr.counts["capture"] == 1 and tr._graph is not None
    ta, tb = [], []
    for _ in range(steps):
        ta.append(timed(ts.step))
        tb.append(timed(tr.step))
    wa, wb = [], []
    for _ in range(3):
        wa.append(block_ms(ts.step, 20))
        wb.append(block_ms(tr.step, 20))
    tr.check_error()
    say(f"{rays} rays x {ts.s_final} samples per step, {steps} alternating steps after warm-up")
    say(f"  (A) bench.TrainStep.step (index copy + graph replay + Adam launch):  {stats(ta)}")
    say(f"  (B) Trainer.step (one graph replay):                               {stats(tb)}")
    say(f"      B - A at the medians: {statistics.median(tb) - statistics.median(ta):+.3f} ms; "
        f"A's min-max spread {max(ta) - min(ta):.3f} ms, B's {max(tb) - min(tb):.3f} ms")
    say(f"  back to back, wall ms per step over 3 blocks of 20:  (A) {stats(wa)};  (B) {stats(wb)}")
    say(f"  trainer steps: {tr.counts}")
    ts.close()
    del ts, tr
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.steps < 20:
        raise SystemExit("train_bench: at least 20 timed steps")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"train_bench: {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    for rays in (4096, 512):
        run_size(rays, a.steps, a.warmup, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
