"""Generate tests/golden/unit_sampling_shapes.npz by running the REFERENCE's samplers
(modules/rendering.py: sample_pdf, sample_3sigma, GenerateGuidedSamples + sort + cat :165-167) on
the CPU, at every size at which the library changes its lane layout.  Seconds:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_sampling_golden.py [--ref /root/reference]

This is the only file of the sampling tests that imports the reference; only data is stored, all
float32 (valid_depth int64).  The draws are recorded with gen_golden.py's Recorder.

    s3_N_{low,high,u,out}                   N in 2, 3, 64, 65, 128, 129, 256; near / far scalars
    pdf_NB_ND_{bins,w,u,out}                (bins, draws) in (1,7) (64,64) (65,100) (128,256) (129,64) (255,300)
    g_MODE_n_{z,depth,w,tdep,tstd,valid,u_pred,u_gt,z2,unsort,sorted}
                                            MODE train (mixed valid_depth) / test, n in 2, 5, 64, 65, 100, 128;
                                            u_gt (valid rays, n) as the reference draws it; z2 = GenerateGuidedSamples
    deg_{low,high,u,out}                    sample_3sigma, N = 8, on zero-width windows: inside [near, far],
                                            at either bound, outside; NaN is stored as NaN
    degg_*                                  as g_train_8_* on four rays: all of pass 1's weight on one sample,
                                            all-zero pass-1 weights (depth 0), target_std = 0 on a valid ray,
                                            and an ordinary ray

Rays per case: 8 to 16.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from gen_golden import Recorder, load_reference  # noqa: E402

NEAR, FAR = 0.02, 0.21
S3_N = (2, 3, 64, 65, 128, 129, 256)
PDF = ((1, 7), (64, 64), (65, 100), (128, 256), (129, 64), (255, 300))
GUIDED_N = (2, 5, 64, 65, 100, 128)
T = torch.tensor


def windows(g, B):
    """inside / tiny / clamped low / clamped high / clamped both / outside below / outside above, then random"""
    c = np.concatenate([[0.1, 0.12, 0.03, 0.2, 0.1, -0.1, 0.4], g.uniform(0.0, 0.25, B - 7)])
    sd = np.concatenate([[0.01, 1e-6, 0.02, 0.02, 0.5, 0.01, 0.05], 10.0 ** g.uniform(-6.0, np.log10(0.5), B - 7)])
    return c.astype(np.float32), sd.astype(np.float32)


def weights(g, B, nb):
    w = g.uniform(0.0, 1.0, (B, nb)).astype(np.float32)
    w[0] = 0.0
    w[1, ::2] = 0.0
    w[2] = 0.0
    w[2, nb // 3] = 1.0
    k = np.arange(nb)
    v = np.exp(-0.5 * ((k - 0.4 * nb) / (0.05 * nb + 0.5)) ** 2)
    w[3] = v / v.sum()
    w[4] = w[4] ** 4
    return w


def run_guided(R, d, train, n):
    """rendering.py:161-167 on the stored inputs; returns (z2, z_vals_unsort, z_vals, recorded draws)"""
    z = T(d["z"])
    res = {"depth": T(d["depth"]), "weights": T(d["w"])}
    near, far = torch.full((z.shape[0], 1), NEAR), torch.full((z.shape[0], 1), FAR)
    with Recorder() as rec:
        z2 = R.GenerateGuidedSamples(res, z, n, 1.0, near, far, mode="train" if train else "test",
                                     valid_depth=T(d["valid"]), target_depths=T(d["tdep"]), target_std=T(d["tstd"]))
    z2s, _ = torch.sort(z2, -1)
    unsort = torch.cat([z, z2s], -1)
    zs, _ = torch.sort(torch.cat([z, z2s], -1), -1)
    return z2, unsort, zs, rec.draws


def guided_inputs(g, B, n):
    z = np.sort(g.uniform(NEAR, FAR, (B, n)), -1).astype(np.float32)
    mu, s = g.uniform(0.03, 0.09, (B, 1)), 10.0 ** g.uniform(-3.0, -1.5, (B, 1))
    v = np.exp(-0.5 * ((z - mu) / s) ** 2) + 1e-9
    v[3] = 1.0                                                   # uniform weights: clamped on both sides
    w = (v / v.sum(-1, keepdims=True) * g.uniform(0.5, 1.0, (B, 1))).astype(np.float32)
    depth = (w.astype(np.float64) * z).sum(-1).astype(np.float32)
    valid = (np.arange(B) % 3 != 1).astype(np.int64)
    gt, gs = g.uniform(0.15, 0.19, B), 10.0 ** g.uniform(-6.0, -2.0, B)
    gt[0], gs[0] = 0.2, 0.02                                     # GT window clamped at far
    gt[3], gs[3] = 0.5, 0.01                                     # wholly outside
    tdep = np.stack([gt, np.ones(B)], 1).astype(np.float32)
    return dict(z=z, depth=depth, w=w, valid=valid, tdep=tdep, tstd=gs.astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(HERE, "unit_sampling_shapes.npz"))
    a = ap.parse_args()
    _, R = load_reference(a.ref)
    store = {"near": np.float32(NEAR), "far": np.float32(FAR)}
    near, far = T(NEAR), T(FAR)

    for N in S3_N:
        g = np.random.default_rng(100 + N)
        torch.manual_seed(100 + N)
        c, sd = windows(g, 12)
        low, high = c - np.float32(3.0) * sd, c + np.float32(3.0) * sd
        with Recorder() as rec:
            out = R.sample_3sigma(T(low), T(high), N, False, near, far)
        assert torch.isfinite(out).all()
        store.update({f"s3_{N}_low": low, f"s3_{N}_high": high, f"s3_{N}_u": rec.draws[0][1].numpy(), f"s3_{N}_out": out.numpy()})

    for nb, nd in PDF:
        g = np.random.default_rng(200 + nb)
        torch.manual_seed(200 + nb)
        bins = np.sort(g.uniform(NEAR, FAR, (10, nb + 1)), -1).astype(np.float32)
        w = weights(g, 10, nb)
        with Recorder() as rec:
            out = R.sample_pdf(T(bins), T(w), nd, det=False)
        assert torch.isfinite(out).all()
        store.update({f"pdf_{nb}_{nd}_bins": bins, f"pdf_{nb}_{nd}_w": w, f"pdf_{nb}_{nd}_u": rec.draws[0][1].numpy(),
                      f"pdf_{nb}_{nd}_out": out.numpy()})

    for n in GUIDED_N:
        for train in (True, False):
            g = np.random.default_rng(300 + n)
            torch.manual_seed(300 + n)
            d = guided_inputs(g, 10, n)
            z2, unsort, zs, drawn = run_guided(R, d, train, n)
            assert torch.isfinite(zs).all() and len(drawn) == (2 if train else 1)
            key = f"g_{'train' if train else 'test'}_{n}_"
            store.update({key + k: v for k, v in d.items()})
            store.update({key + "u_pred": drawn[0][1].numpy(), key + "z2": z2.numpy(), key + "unsort": unsort.numpy(),
                          key + "sorted": zs.numpy()})
            if train:
                store[key + "u_gt"] = drawn[1][1].numpy()

    # degenerate windows: what the reference returns there, NaN included
    torch.manual_seed(7)
    c = np.array([0.1, 0.0, NEAR, FAR, -0.1, 0.3, 0.1, 0.15], np.float32)
    with Recorder() as rec, np.errstate(all="ignore"):
        out = R.sample_3sigma(T(c), T(c), 8, False, near, far)
    store.update(deg_low=c, deg_high=c, deg_u=rec.draws[0][1].numpy(), deg_out=out.numpy())
    print("sample_3sigma on zero-width windows:", out.numpy())

    g = np.random.default_rng(8)
    torch.manual_seed(8)
    n = 8
    d = guided_inputs(g, 8, n)
    d["valid"] = np.array([0, 0, 1, 0, 0, 0, 1, 0], np.int64)
    d["w"][0] = 0.0
    d["w"][0, 3] = 1.0
    d["depth"][0] = d["z"][0, 3]                                  # all weight on one sample
    d["w"][1] = 0.0
    d["depth"][1] = 0.0                                           # an empty ray
    d["tstd"][2] = 0.0                                            # GT spread 0 on a valid ray
    d["tdep"][2, 0] = 0.17
    d["w"][4] = 0.0
    d["w"][4, 0] = 1.0
    d["depth"][4] = d["z"][4, 0]
    z2, unsort, zs, drawn = run_guided(R, d, True, n)
    store.update({"degg_" + k: v for k, v in d.items()})
    store.update(degg_u_pred=drawn[0][1].numpy(), degg_u_gt=drawn[1][1].numpy(), degg_z2=z2.numpy(),
                 degg_unsort=unsort.numpy(), degg_sorted=zs.numpy())
    print("GenerateGuidedSamples on the degenerate rays:", z2.numpy())

    for k, v in store.items():
        assert np.asarray(v).dtype in (np.float32, np.int64), (k, np.asarray(v).dtype)
    np.savez_compressed(a.out, **store)
    print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
