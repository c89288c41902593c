"""Time a whole-view render with all image products on one GPU: a 1024 x 1024 crop of the C5
camera (JAX_269_006 RPC at x5), C5 flags (128 stratified samples, semantic head, W = 512, bf16 MLP),
chunks of 32768 rays, on-device draws.  Device events, median of the calls after warm-up.

  (a) ``render_image`` with every product, then ``view_metrics``;
  (b) the same planes the way it had to be done before: the ``render_rays`` chunk loop keeping the
      per-sample dictionary, then the reference's ``torch.sum(weights.unsqueeze(-1) * x, -2)``
      expressions and ``argmax`` (eval.py:63, 76-101), in the same process;
  (c) ``k_composite_products`` against ``k_composite_fwd``, per launch on one chunk's rows, the
      two alternating, with the achieved GB/s over the algorithmic byte count (the rows and depths
      are fp32: 4-byte operands), and ``k_view_metrics`` + finish on the whole view.

    python tools/view_bench.py [--side 1024] [--calls 10] [--warmup 2] [--out profiles/r10/view.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def stats(ms):
    return f"median {statistics.median(ms):.3f} ms, min {min(ms):.3f} ms, max {max(ms):.3f} ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=32768)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bench
    import spnerf_amd
    from spnerf_amd import PhiloxRandom, _lib, random_source, view
    from spnerf_amd.satellite import image_rays, load_cameras
    from spnerf_amd.spnerf import _Composite, run_mlp

    dev = torch.device("cuda", 0)
    c = bench.CONFIGS["c5"]
    args = bench.make_args(c)
    cams = load_cameras()
    rays = image_rays(cams["images"][c["view"]], c["img_downscale"], cams["scene_loc"], crop=(0, 0, a.side, a.side), device=dev)
    n, S, B = rays.shape[0], args.n_samples, a.chunk
    gid = torch.arange(n, device=dev, dtype=torch.int64)
    sems = (gid * 0x9E3779B1 & 0xFFFFFFFF) % 3
    torch.manual_seed(0)
    model = spnerf_amd.SPNeRF(num_sem_classes=3, layers=8, feat=512, mapping=True, sem=True, precision=c["precision"]).to(dev)
    models = {"coarse": model}
    C, NO = 3, model.number_of_outputs
    names = ("rgb", "depth", "sun", "albedo", "sky", "sem_logits", "sem_class")
    new = {k: torch.empty((n,) + view._PLANES[k][0](C), dtype=view._PLANES[k][1], device=dev) for k in names}
    old = {k: torch.empty_like(v) for k, v in new.items()}

    def render_new():
        with random_source(PhiloxRandom(seed=0)):
            spnerf_amd.render_image(models, args, rays, None, sems, chunk=B, out=new)

    @torch.no_grad()
    def render_old():
        src = PhiloxRandom(seed=0)
        with random_source(src):
            for i0 in range(0, n, B):
                i1 = min(n, i0 + B)
                src.ray_offset = i0
                src.reset_step(-1)
                r = spnerf_amd.render_rays(models, args, rays[i0:i1], None, semantics=sems[i0:i1], mode="test")
                w = r["weights_coarse"].unsqueeze(-1)
                old["rgb"][i0:i1], old["depth"][i0:i1] = r["rgb_coarse"], r["depth_coarse"]
                old["sun"][i0:i1] = torch.sum(w * r["sun_coarse"], -2).squeeze(-1)
                old["albedo"][i0:i1] = torch.sum(w * r["albedo_coarse"], -2)
                old["sky"][i0:i1] = torch.sum(w * r["sky_coarse"], -2)
                old["sem_logits"][i0:i1] = r["sem_logits_coarse"]
                old["sem_class"][i0:i1] = r["sem_logits_coarse"].argmax(-1)

    ms_new, ms_old = [], []
    for _ in range(a.warmup):
        render_new()
        render_old()
    for _ in range(a.calls):      # alternating, so that both see the same machine
        ms_new += timed(render_new, 1, 0)
        ms_old += timed(render_old, 1, 0)
    same = {k: bool(torch.equal(new[k], old[k])) for k in ("rgb", "depth", "sem_logits", "sem_class")}
    rel = {k: float((new[k] - old[k]).norm() / old[k].norm()) for k in ("sun", "albedo", "sky")}

    # (c) one chunk's rows through both compositing kernels
    # (the library's own timer: device events around the launch itself, no host path in between)
    with torch.no_grad():
        z = spnerf_amd.stratified(rays[:B], S, torch.rand(B, S, device=dev))
        rows = run_mlp(model, rays[:B], z, 3, sems[:B])
    planes = {k: v[:B] for k, v in new.items()}
    ms_c, ms_p = [], []

    def launch(cls, fn):
        _lib.prof_reset()
        fn()
        return _lib.prof_read(cls)["ms"]

    fwd = lambda: _Composite.apply(rows, z, None, 0.0, 8, C, False)               # noqa: E731
    prod = lambda: view.composite_products(model, rows, z, 0.0, planes)           # noqa: E731
    _lib.prof_enable(True)
    for i in range(a.warmup + a.calls):
        c_ms, p_ms = launch("composite_fwd", fwd), launch("composite_products", prod)
        if i >= a.warmup:
            ms_c.append(c_ms)
            ms_p.append(p_ms)
    _lib.prof_enable(False)
    P = B * S
    load = P * (NO * 4 + 4)
    by_c = load + P * 8 + B * 4 * (3 + 1 + C)
    by_p = load + B * 4 * (3 + 1 + 1 + 3 + 3 + C + 1)
    target = (new["rgb"] + 0.05).clamp(0, 1)
    score = lambda: spnerf_amd.view_metrics(new, target, labels=sems, num_classes=C)   # noqa: E731
    ms_m = timed(score, a.calls, a.warmup)
    _lib.prof_enable(True)
    ms_mk = [launch("view_metrics", score) for _ in range(a.calls)]
    _lib.prof_enable(False)
    m = spnerf_amd.view_metrics(new, target, labels=sems, num_classes=C)
    by_m = n * (24 + 12)
    mc, mp = statistics.median(ms_c), statistics.median(ms_p)
    lines = [
        f"whole view {a.side} x {a.side} = {n} rays x {S} samples, W=512 {c['precision']} MLP, C={C}, chunks of {B} rays, "
        f"{torch.cuda.get_device_name(0)}; device events, {a.calls} calls after {a.warmup} warm-up, (a)/(b) and the two "
        f"kernels of (c) alternating",
        f"(a) render_image, all products:                  {stats(ms_new)}",
        f"(b) render_rays loop + torch.sum / argmax:        {stats(ms_old)}",
        f"    (b) / (a) = {statistics.median(ms_old) / statistics.median(ms_new):.3f} (medians)",
        f"    planes (a) == (b) bit for bit: {same}; norm-relative difference of the reordered sums: "
        + ", ".join(f"{k} {v:.1e}" for k, v in rel.items()),
        f"(c) per launch on one chunk ({B} rays x {S} samples x {NO} fp32 outputs):",
        f"    k_composite_fwd      {stats(ms_c)}; {by_c / 1e6:.1f} MB -> {by_c / mc / 1e6:.0f} GB/s",
        f"    k_composite_products {stats(ms_p)}; {by_p / 1e6:.1f} MB -> {by_p / mp / 1e6:.0f} GB/s",
        f"    products - composite = {mp - mc:+.4f} ms (medians); the composite's own min-to-max spread {max(ms_c) - min(ms_c):.4f} ms",
        f"k_view_metrics + finish, {n} rays: {stats(ms_mk)}; {by_m / 1e6:.1f} MB -> "
        f"{by_m / statistics.median(ms_mk) / 1e6:.0f} GB/s",
        f"view_metrics end to end (allocations, both kernels, the one copy to the host): {stats(ms_m)}; "
        f"psnr {m['psnr']:.4f} miou {m['miou']:.4f} oa {m['oa']:.4f}",
    ]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
