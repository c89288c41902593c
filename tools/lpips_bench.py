"""Time ``spnerf_amd.lpips`` on one GPU on a 1024 x 1024 pair, against the same definition in fp32
torch on the GPU.

  (A) ``spnerf_amd.lpips`` (csrc/lpips.hip): im2col gathers + the fp32 MFMA GEMM, pools, the
      distance kernel and the finish, at three workspace caps: none (no convolution split), the
      default 256 MiB, and 64 MiB;
  (B) tests/lpips_torch.py's restatement with dtype float32 on the device (torch's own convolutions).

Device events around batches of ``--batch`` calls, the arms alternating batch by batch after a
warm-up of all; per-call time = batch time / batch; median with min and max.  Last, the scores and
how far each lies from the fp64 restatement on the CPU, weights seeded as in the tests.

    python tools/lpips_bench.py [--side 1024] [--pairs 7] [--batch 5] [--warmup 2] [--out bench_out/lpips.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def batch_ms(fn, batch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(batch):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / batch


def stats(ms):
    return f"median {statistics.median(ms):.3f} ms, min {min(ms):.3f} ms, max {max(ms):.3f} ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--batch", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import lpips_torch as lt
    import spnerf_amd
    from spnerf_amd import perceptual

    dev = torch.device("cuda", 0)
    H = W = a.side
    cpu_w = lt.seeded_weights()
    w = spnerf_amd.LpipsWeights.from_tensors(*cpu_w, device=dev)
    dev_w = tuple(tuple(t.to(dev) for t in seq) for seq in cpu_w)
    x, y = lt.pair(H, W)
    xd, yd = x.to(dev), y.to(dev)
    full = perceptual.workspace_bytes(H, W, 0)
    caps = (("no cap", 0), ("256 MiB", 256 << 20), ("64 MiB", 64 << 20))
    arms = {f"(A) spnerf_amd.lpips, {name}": (lambda cap=cap: spnerf_amd.lpips(xd, yd, w, layout="chw", max_workspace_bytes=cap))
            for name, cap in caps}
    arms["(B) torch fp32 on the device"] = lambda: lt.lpips(xd, yd, dev_w, dtype=torch.float32)[0]
    for _ in range(a.warmup):
        for fn in arms.values():
            batch_ms(fn, a.batch)
    ms = {k: [] for k in arms}
    for _ in range(a.pairs):
        for k, fn in arms.items():
            ms[k].append(batch_ms(fn, a.batch))
    lines = [f"lpips of one {H} x {W} pair in [0, 1] (uniform noise against itself + N(0, 0.25), clamped), "
             f"{torch.cuda.get_device_name(0)}; device events around batches of {a.batch} calls, {a.pairs} rounds of all arms "
             f"after {a.warmup} warm-up rounds; times per call; whole workspace {full / 2 ** 20:.0f} MiB"]
    for (name, cap), k in zip(caps, arms):
        n = perceptual.workspace_bytes(H, W, cap)
        lines.append(f"  {k}: {stats(ms[k])}; workspace {n / 2 ** 20:.0f} MiB, bands {perceptual.bands(H, W, n)}")
    k = "(B) torch fp32 on the device"
    lines.append(f"  {k}: {stats(ms[k])}")
    ref = lt.lpips(x, y, cpu_w)[0]
    got = [float(fn()) for fn in arms.values()]
    lines.append(f"  fp64 restatement on the CPU: {ref:.12e}")
    for k, v in zip(arms, got):
        lines.append(f"  {k}: {v:.12e}  relative deviation {abs(v - ref) / ref:.1e}")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
