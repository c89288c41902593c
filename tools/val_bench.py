"""Time the solar march of a whole view on one GPU: a 256 x 256 crop of the C5 camera at the C5
model size (W = 512, bf16 MLP, 128 stratified samples, guided sampling off) with ``sc_lambda`` 0.1,
on-device draws, rendered with and without the "sc" product in the same process, the two
alternating.  Device events, median of the calls after warm-up; the solar-terms kernel and the loss
reduction through the library's own timer, with the achieved GB/s over the algorithmic byte count.

    python tools/val_bench.py [--side 256] [--calls 10] [--warmup 2] [--out profiles/r15/val.txt]
"""
import argparse
import os
import statistics
import sys

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bench
    import spnerf_amd
    from spnerf_amd import PhiloxRandom, _lib, random_source
    from spnerf_amd.satellite import image_rays, load_cameras

    dev = torch.device("cuda", 0)
    c = bench.CONFIGS["c5"]
    args = bench.make_args(c)
    args.sc_lambda, args.guidedsample = 0.1, False
    cams = load_cameras()
    rays = image_rays(cams["images"][c["view"]], c["img_downscale"], cams["scene_loc"], crop=(0, 0, a.side, a.side), device=dev)
    n, S = rays.shape[0], args.n_samples
    sems = (torch.arange(n, device=dev, dtype=torch.int64) * 0x9E3779B1 & 0xFFFFFFFF) % 3
    torch.manual_seed(0)
    model = spnerf_amd.SPNeRF(num_sem_classes=3, layers=8, feat=512, mapping=True, sem=True, precision=c["precision"]).to(dev)
    models = {"coarse": model}
    target = torch.rand(n, 3, device=dev)
    base = ("rgb", "depth", "sun", "albedo", "sky", "sem")
    res = {}

    def render(products):
        with random_source(PhiloxRandom(seed=0)):
            res[products] = spnerf_amd.render_image(models, args, rays, None, sems, products=products)

    ms = {base: [], base + ("sc",): []}
    for _ in range(a.warmup):
        for p in ms:
            render(p)
    for _ in range(a.calls):      # alternating, so that both see the same machine
        for p in ms:
            ms[p].append(timed(lambda: render(p)))
    same = all(torch.equal(res[base][k], res[base + ("sc",)][k]) for k in res[base])
    # the kernels of the last call with the product, and the loss, through the library's timer
    torch.cuda.synchronize()
    _lib.prof_reset()
    _lib.prof_enable(True)
    for _ in range(a.calls):
        render(base + ("sc",))
        loss = spnerf_amd.view_metrics(res[base + ("sc",)], target, loss=dict(lambda_sc=args.sc_lambda))
    torch.cuda.synchronize()
    _lib.prof_enable(False)
    prof = {k: _lib.prof_read(k) for k in _lib.prof_classes()}
    med_off, med_on = statistics.median(ms[base]), statistics.median(ms[base + ("sc",)])
    NO = model.number_of_outputs
    lines = [f"val_bench: {a.side} x {a.side} view ({n} rays), W = 512 {c['precision']}, S' = {S}, guided off, sc_lambda 0.1, "
             f"{a.calls} calls after {a.warmup} warm-up, device {torch.cuda.get_device_name(0)}",
             f"render_image without sc: {stats(ms[base])}",
             f"render_image with sc:    {stats(ms[base + ('sc',)])}",
             f"ratio with / without: {med_on / med_off:.3f}; the other planes bit-identical: {same}",
             f"bytes per sample of val_solar_terms: {NO * 4 + 4} (a row of {NO} floats and a depth, read once) + 8 B per ray written"]
    for k in sorted(prof):
        p = prof[k]
        if p["launches"]:
            per = p["ms"] / p["launches"]
            gbs = f", {p['bytes'] / p['launches'] / per / 1e6:.0f} GB/s" if p["bytes"] else ""
            lines.append(f"  {k}: {p['launches'] // a.calls} launches per call, {per:.4f} ms per launch{gbs}")
    lines.append(f"view_metrics(loss=): {loss['loss']:.6f} = " + " + ".join(f"{k} {v:.6f}" for k, v in loss.items()
                                                                             if k.startswith("coarse_")))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.join(ROOT, a.out)), exist_ok=True)
        with open(os.path.join(ROOT, a.out), "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
