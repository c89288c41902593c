"""Time forward + backward of ``spnerf_amd.FusedTrainLoss`` on one GPU against the sum of the torch
classes of ``spnerf_amd.losses`` on the same tensors: β colour + solar terms + GNLL depth +
semantics, coarse pass only, B = 4096 and B = 512 rays of S = 128 samples, C = 5 classes.

  (A) ``FusedTrainLoss(lambda_sc, beta=True, lambda_ds, GNLL=True, lambda_ss)``: k_tl_rays +
      k_tl_final forward, k_tl_grad backward (csrc/train_loss.hip);
  (B) ``SatNerfLoss + DepthLoss(GNLL=True, usealldepth=False) + SemanticLoss`` and autograd.

Inputs are render-shaped: ``sun_sc`` and ``beta`` are columns of one (B·S, 11) buffer, and the
gradients are taken with respect to rgb, depth, weights, the logits and that buffer, as a render's
backward would receive them.  A step is loss + ``torch.autograd.grad``.  Device events around
batches of ``--batch`` steps, the two arms alternating batch by batch after ``--warmup`` batches of
each; per-step time = batch time / batch; median, min and max over the ``--pairs`` batches.  The
spread of an arm is max - min; (A) counts as faster when median(B) - median(A) exceeds the larger
of the two spreads.  (A)'s kernels alone come from the library's own timer (device events around
the launches).  Both arms' values are compared once before timing.

A batch whose per-step time exceeds ``--step-limit-ms`` ends the run with an error; run the
command itself under ``timeout`` as well, since a launch that never returns cannot be seen from here.

    timeout -k 10 300 python tools/loss_bench.py [--pairs 15] [--batch 200] [--warmup 3] [--out profiles/r12/loss_bench.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NO, SUN_COL, BETA_COL = 11, 4, 8
LSC, LDS, LSS = 0.05, 1.0, 0.04


def inputs(B, S, C, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, device=dev, generator=g)   # noqa: E731
    wide = rnd(B * S, NO).requires_grad_(True)
    w = rnd(B, S) ** 3
    w = w / w.sum(1, keepdim=True) * (0.6 + 0.4 * rnd(B, 1))
    z = torch.sort(rnd(B, S) * 0.2, 1)[0]
    x = {"rgb_coarse": rnd(B, 3).requires_grad_(True), "depth_coarse": (w * z).sum(1).requires_grad_(True),
         "weights_coarse": w.requires_grad_(True), "z_vals_coarse": z,
         "sem_logits_coarse": torch.randn(B, C, device=dev, generator=g).requires_grad_(True),
         "transparency_sc_coarse": torch.cumprod(0.8 + 0.2 * rnd(B, S), 1), "weights_sc_coarse": 0.1 * rnd(B, S),
         "sun_sc_coarse": wide.view(B, S, NO)[..., SUN_COL:SUN_COL + 1],
         "beta_coarse": wide.view(B, S, NO)[..., BETA_COL:BETA_COL + 1]}
    td = torch.stack([x["depth_coarse"].detach() * (0.7 + 0.6 * rnd(B)), 0.2 + 0.8 * rnd(B)], 1)
    t = dict(targets=rnd(B, 3), td=td, valid=(rnd(B) < 0.7).long(),
             tstd=torch.where(rnd(B) < 0.5, 0.15 + 0.1 * rnd(B), 1e-3 + 0.02 * rnd(B)),
             labels=torch.where(rnd(B) < 0.15, torch.full((B,), -100, device=dev),
                                torch.randint(0, C, (B,), device=dev, generator=g)))
    wrt = [x["rgb_coarse"], x["depth_coarse"], x["weights_coarse"], x["sem_logits_coarse"], wide]
    return x, t, wrt


def batch_ms(fn, batch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(batch):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / batch


def stats(ms):
    return (f"median {statistics.median(ms) * 1e3:.1f} us, min {min(ms) * 1e3:.1f} us, max {max(ms) * 1e3:.1f} us, "
            f"spread {(max(ms) - min(ms)) * 1e3:.1f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=15)
    ap.add_argument("--batch", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--classes", type=int, default=5)
    ap.add_argument("--step-limit-ms", type=float, default=100.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("loss_bench: no GPU: nothing is measured on the CPU")
    from spnerf_amd import _lib
    from spnerf_amd import losses as L

    dev = torch.device("cuda", 0)
    S, C = a.samples, a.classes
    lines = [f"training loss, forward + backward: beta colour + solar + GNLL depth + semantics, coarse pass, S = {S}, C = {C}, "
             f"{torch.cuda.get_device_name(0)}; device events around batches of {a.batch} steps, {a.pairs} alternating "
             f"(A)/(B) pairs after {a.warmup} warm-up batches of each; times per step"]
    ok = True
    for B in (4096, 512):
        x, t, wrt = inputs(B, S, C, dev)
        fused = L.FusedTrainLoss(LSC, True, LDS, GNLL=True, lambda_ss=LSS)
        sat, dl, ce = L.SatNerfLoss(lambda_sc=LSC), L.DepthLoss(LDS, GNLL=True, usealldepth=False), L.SemanticLoss(LSS)

        def arm_a():
            loss, _ = fused(x, t["targets"], t["td"], t["valid"], t["tstd"], t["labels"])
            return loss, torch.autograd.grad(loss, wrt)

        def arm_b():
            loss = (sat(x, t["targets"])[0] + dl(x, t["td"][:, 0], t["td"][:, 1], t["valid"], t["tstd"])[0]
                    + ce(x, t["labels"])[0])
            return loss, torch.autograd.grad(loss, wrt)

        (la, ga), (lb, gb) = arm_a(), arm_b()
        err = max(float((p - q).abs().max() / q.abs().max()) for p, q in zip(ga, gb))
        lines.append(f"B = {B}: loss (A) {float(la):.7f}  (B) {float(lb):.7f}; largest gradient difference / max |gradient| = {err:.1e}")
        ms_a, ms_b = [], []
        for i in range(a.warmup + a.pairs):
            pa, pb = batch_ms(arm_a, a.batch), batch_ms(arm_b, a.batch)
            if max(pa, pb) > a.step_limit_ms:
                sys.exit(f"loss_bench: a step took {max(pa, pb):.1f} ms, over the limit of {a.step_limit_ms} ms")
            if i >= a.warmup:
                ms_a.append(pa)
                ms_b.append(pb)
        kern = []
        _lib.prof_enable(True)
        for i in range(a.warmup + a.pairs):
            _lib.prof_reset()
            arm_a()
            torch.cuda.synchronize()
            if i >= a.warmup:
                kern.append(_lib.prof_read("train_loss")["ms"])
        _lib.prof_enable(False)
        ma, mb = statistics.median(ms_a), statistics.median(ms_b)
        spread = max(max(ms_a) - min(ms_a), max(ms_b) - min(ms_b))
        faster = mb - ma > spread
        ok = ok and faster
        lines += [
            f"  (A) FusedTrainLoss (2 + 1 launches):                    {stats(ms_a)}",
            f"  (B) SatNerfLoss + DepthLoss(GNLL) + SemanticLoss, torch: {stats(ms_b)}",
            f"      (B) / (A) = {mb / ma:.2f} (medians); (B) - (A) = {(mb - ma) * 1e3:.1f} us against a spread of "
            f"{spread * 1e3:.1f} us: (A) is {'faster' if faster else 'NOT faster'} by more than the spread; "
            f"(A) faster in {sum(p < q for p, q in zip(ms_a, ms_b))} of {a.pairs} pairs",
            f"  (A) kernels alone (3 launches, the library's events): median {statistics.median(kern) * 1e3:.1f} us, "
            f"min {min(kern) * 1e3:.1f} us, max {max(kern) * 1e3:.1f} us",
        ]
    lines.append("verdict: the fused arm is " + ("faster at both sizes by more than the spread" if ok
                                                 else "NOT faster by more than the spread at every size"))
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
