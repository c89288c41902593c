"""Time ``spnerf_amd.ssim`` on one GPU against what the reference runs, moved to the GPU, on
1024 x 1024 x 3 images at window sizes 3 (the reference's) and 11.

  (A) ``spnerf_amd.ssim``: k_ssim_tiles + k_ssim_finish, fp64 (csrc/ssim.hip);
  (B) the definition of include/spnerf_amd_image.h in fp32 torch: ``F.pad(mode='reflect')`` + a
      grouped ``conv2d`` for each of the five filtered images, the elementwise map, ``mean`` —
      the window is built once, outside the timed region.

Device events around batches of ``--batch`` calls, the two arms alternating batch by batch after a
warm-up of both; per-call time = batch time / batch; median with min and max over the pairs, and in
how many pairs (A) was the faster.  (A)'s two kernels alone come from the library's own timer
(device events around the launches), with the achieved GB/s over the byte model 2·C·H·W·4 bytes
read, plus C·H·W·8 when the map is stored.  Last, how far (B)'s fp32 score and map lie from (A)'s
on the timed noise images and on one smooth synthetic image (sinusoid / ramp / constant planes,
target = image + 0.01).

    python tools/ssim_bench.py [--side 1024] [--pairs 15] [--batch 20] [--warmup 3] [--out profiles/r11/ssim.txt]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window(ws, C, device):
    i = torch.arange(ws, dtype=torch.float32, device=device) - ws // 2
    g = torch.exp(-(i * i) / (2 * 1.5 ** 2))
    g = g / g.sum()
    return torch.outer(g, g).expand(C, 1, ws, ws).contiguous()


def torch_ssim(x, y, k, max_val=1.0):
    """(score, map) of (1, C, H, W) fp32 images: arm (B)."""
    C, r = x.shape[1], k.shape[-1] // 2
    f = lambda t: F.conv2d(F.pad(t, (r, r, r, r), mode="reflect"), k, groups=C)   # noqa: E731
    c1, c2 = (0.01 * max_val) ** 2, (0.03 * max_val) ** 2
    mu1, mu2 = f(x), f(y)
    s1, s2, s12 = f(x * x) - mu1 * mu1, f(y * y) - mu2 * mu2, f(x * y) - mu1 * mu2
    m = ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2) + 1e-12)
    return m.mean(), m


def batch_ms(fn, batch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(batch):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / batch


def stats(ms, unit=1e3):
    return f"median {statistics.median(ms) * unit:.1f} us, min {min(ms) * unit:.1f} us, max {max(ms) * unit:.1f} us"


def smooth_pair(side, device):
    """A smooth image in [0, 1] (a sinusoid, a ramp and a constant plane) and image + 0.01."""
    i = torch.arange(side, dtype=torch.float64, device=device)
    yy, xx = torch.meshgrid(i, i, indexing="ij")
    x = torch.stack([0.5 + 0.4 * torch.sin(xx / 9.0) * torch.cos(yy / 13.0), (xx + yy) / (2.5 * side) + 0.1,
                     torch.full_like(xx, 0.3)])[None].float()
    return x, x + 0.01


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--pairs", type=int, default=15)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import spnerf_amd
    from spnerf_amd import _lib

    dev = torch.device("cuda", 0)
    C, H, W = 3, a.side, a.side
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand((1, C, H, W), device=dev, generator=g)
    y = (x + 0.1 * torch.randn((1, C, H, W), device=dev, generator=g)).clamp(0, 1)
    values = C * H * W
    lines = [f"ssim of {H} x {W} x {C} fp32 images in [0, 1] (uniform noise against itself + N(0, 0.1), clamped), "
             f"{torch.cuda.get_device_name(0)}; device events around batches of {a.batch} calls, {a.pairs} alternating "
             f"(A)/(B) pairs after {a.warmup} warm-up batches of each; times per call"]
    for ws in (3, 11):
        k = window(ws, C, dev)
        arm_a = lambda: spnerf_amd.ssim(x, y, window_size=ws)         # noqa: E731
        arm_b = lambda: torch_ssim(x, y, k)[0]                       # noqa: E731
        for _ in range(a.warmup):
            batch_ms(arm_a, a.batch)
            batch_ms(arm_b, a.batch)
        ms_a, ms_b = [], []
        for _ in range(a.pairs):
            ms_a.append(batch_ms(arm_a, a.batch))
            ms_b.append(batch_ms(arm_b, a.batch))
        wins = sum(p < q for p, q in zip(ms_a, ms_b))
        # (A)'s kernels alone, with and without the map
        smap = torch.empty((C, H, W), dtype=torch.float64, device=dev)
        res = torch.zeros(6, dtype=torch.float64, device=dev)
        kern = {}
        _lib.prof_enable(True)
        for name, mp in (("no map", None), ("map stored", smap)):
            t = []
            for i in range(a.warmup + a.pairs):
                _lib.prof_reset()
                spnerf_amd.image.launch_ssim(x[0], y[0], C, H, W, x[0].stride(), ws, 1.0, res.data_ptr(), mp)
                torch.cuda.synchronize()
                if i >= a.warmup:
                    t.append(_lib.prof_read("image_ssim")["ms"])
            kern[name] = t
        _lib.prof_enable(False)
        sa, (sb, mb) = spnerf_amd.ssim(x, y, window_size=ws, return_map=True), torch_ssim(x, y, k)
        ma, mb_ = statistics.median(ms_a), statistics.median(ms_b)
        lines += [
            f"ws {ws}:",
            f"  (A) spnerf_amd.ssim (2 launches, fp64):           {stats(ms_a)}",
            f"  (B) pad + grouped conv2d x 5 + map + mean (fp32): {stats(ms_b)}",
            f"      (B) / (A) = {mb_ / ma:.2f} (medians); (A) faster in {wins} of {a.pairs} pairs",
        ]
        for name, t in kern.items():
            by = values * (8 + (8 if name == "map stored" else 0))
            lines.append(f"  (A) kernels alone, {name}: {stats(t)}; {by / 1e6:.1f} MB -> {by / statistics.median(t) / 1e6:.0f} GB/s")
        lines.append(f"  scores: (A) {float(sa[0]):.12f}  (B) {float(sb):.12f}  (B) - (A) = {float(sb) - float(sa[0]):+.2e}; "
                     f"map max |(B) - (A)| = {float((mb[0].double() - sa[1]).abs().max()):.2e}")
        xs, ys = smooth_pair(a.side, dev)
        sa, (sb, mb) = spnerf_amd.ssim(xs, ys, window_size=ws, return_map=True), torch_ssim(xs, ys, k)
        lines.append(f"  smooth image (sinusoid / ramp / constant planes, target = image + 0.01): (A) {float(sa[0]):.12f}  "
                     f"(B) {float(sb):.12f}  (B) - (A) = {float(sb) - float(sa[0]):+.2e}; "
                     f"map max |(B) - (A)| = {float((mb[0].double() - sa[1]).abs().max()):.2e}")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
