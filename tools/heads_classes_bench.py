"""Time a bf16 training step and an inference render at 3 and at 5 semantic classes on one GPU.

bench.py builds its model with three classes; the reference trainer's default is five.  Per class
count C in {3, 5}, W = 512, 8 layers, bf16, solar correction on:

  * one training step — guided render of 64 + 64 samples per ray, a fixed scalar loss (the mean
    square of every differentiable output), backward — at 4 096 and at 512 rays;
  * one inference render (mode "test", no grad) of 32 768 rays x 128 samples.

Device events around each step, ``--warmup`` steps first, then the median, min and max of
``--steps``.  The library's profiling classes of one further step tell which heads ran (heads_train /
trunk_heads_bf16 = the fused kernels, heads_fwd = the wave-per-point heads) and heads_bwd_path which
heads backward (1 = the fused dX launch).

``--lib`` names the build under sp-nerf_amd/ to load, so two builds are compared by running this
tool once per build, alternating, in one job (one process per library):

    for i in 1 2 3 4; do for lib in libspnerf_amd_prev.so libspnerf_amd.so; do
      timeout -k 10 300 python tools/heads_classes_bench.py --lib $lib --out profiles/r14/heads_classes_bench.txt || exit 1
    done; done

A step over ``--step-limit-ms`` ends the run with an error; run the command under ``timeout`` too.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default="libspnerf_amd.so")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--classes", type=int, nargs="+", default=[3, 5])
    ap.add_argument("--step-limit-ms", type=float, default=2000.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.environ["SPNERF_AMD_LIB"] = a.lib
    import torch
    if not torch.cuda.is_available():
        sys.exit("heads_classes_bench: no GPU: nothing is measured on the CPU")
    import golden_util as gu
    import spnerf_amd
    from spnerf_amd import _lib

    dev = torch.device("cuda", 0)
    lines = [f"lib {a.lib}, {torch.cuda.get_device_name(0)}: W = 512, bf16; device events per step, "
             f"{a.warmup} warm-up steps, then {a.steps} steps (median / min / max ms)"]

    def timed(name, step):
        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.steps):
            ms.append(event_ms(step))
            if ms[-1] > a.step_limit_ms:
                sys.exit(f"heads_classes_bench: a step took {ms[-1]:.1f} ms, over the limit of {a.step_limit_ms} ms")
        _lib.set_option("heads_bwd_path", 0)
        _lib.prof_reset()
        _lib.prof_enable(True)
        step()
        torch.cuda.synchronize()
        _lib.prof_enable(False)
        heads = {c: round(_lib.prof_read(c)["ms"], 3) for c in _lib.prof_classes() if c.startswith(("heads", "trunk_heads"))}
        lines.append(f"  {name}: median {statistics.median(ms):.3f}  min {min(ms):.3f}  max {max(ms):.3f} ms; "
                     f"heads classes (ms) {heads}, heads_bwd_path {_lib.get_option('heads_bwd_path')}")

    for C in a.classes:
        model = spnerf_amd.SPNeRF(num_sem_classes=C, layers=8, feat=512, mapping=True, sem=True, precision="bf16").to(dev)
        for B in (4096, 512):
            g = torch.Generator(device="cpu").manual_seed(1)
            rays = torch.tensor(gu.synthetic_rays(B, 3), device=dev)
            args = gu.args_of({"args": dict(n_samples=64, n_importance=0, model="sp-nerf", beta=False, guidedsample=True,
                                            sc_lambda=0.1, margin=1e-4, stdscale=1.0, chunk=5120, noise_std=0.0)})
            kw = dict(valid_depth=(torch.rand(B, generator=g) < 0.7).long().to(dev),
                      target_depths=torch.stack([rays[:, 7] * 0.5, torch.ones(B, device=dev)], 1),
                      target_std=torch.full((B,), 0.01, device=dev))
            labels = torch.randint(0, C, (B,), generator=g).to(dev)

            def train_step():
                model.zero_grad(set_to_none=True)
                res = spnerf_amd.render_rays({"coarse": model}, args, rays, None, semantics=labels, mode="train", **kw)
                loss = sum((v.float() ** 2).mean() for k, v in sorted(res.items()) if v.requires_grad)
                loss.backward()

            timed(f"C = {C}, training step, {B} rays x (64 + 64 guided)", train_step)
        B, S = 32768, 128
        g = torch.Generator(device="cpu").manual_seed(2)
        rays = torch.tensor(gu.synthetic_rays(B, 5), device=dev)
        labels = torch.randint(0, C, (B,), generator=g).to(dev)
        iargs = gu.args_of({"args": dict(n_samples=S, n_importance=0, model="sp-nerf", beta=False, guidedsample=False,
                                         sc_lambda=0.0, margin=1e-4, stdscale=1.0, chunk=5120, noise_std=0.0)})

        def infer_step():
            with torch.no_grad():
                spnerf_amd.render_rays({"coarse": model}, iargs, rays, None, semantics=labels, mode="test")

        timed(f"C = {C}, inference render, {B} rays x {S}", infer_step)
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
