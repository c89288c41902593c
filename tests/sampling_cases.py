"""Inputs, tolerance and measured constants shared by tests/test_sampling_ref.py (CPU) and
tests/test_gpu_sampling.py (MI355X): every case is built here once, from fixed seeds, so the CPU
module vets exactly what the GPU module runs.

The value bound of a drawn sample s (float64 restatement, tests/sampling_numpy.py):

    |got - s| <= K 2^-24 bw / den + 4 2^-24 |s|

The first term is the CDF's rounding error carried through the interpolation (bw / den is the
inverse CDF's slope in the selected bin), the second the final float32 operations.  K is not chosen:
K_ORACLE lists, per shape, the K the float32 torch oracle (oracle/ref_cpu.py, pinned to the
reference by tests/test_oracle_golden.py) needs against the restatement on these inputs, rounded up
to two digits; the kernels get twice that.  They accumulate the CDF in double, so they should need
less than the oracle; they sum the normaliser in another order (a wave tree), which is all the
factor of two pays for.  K is 0 where the CDF is exact in float32 (one bin, or two equal ones): the
second term alone holds there.  The table is printed by

    PYTHONPATH=.:tests python tests/sampling_cases.py

Draws the ambiguity mask marks (sampling_numpy's docstring) are left out of the value bound, at
most MAX_LEFT_OUT of a case and half of any row; each must still be finite and lie in its tiny
bins' hull [lo, hi], widened by what a draw within delta of the hull's ends moves by (interval()).

The guided kernel returns its samples sorted, which loses the draw a sample came from; the
per-draw bound is applied rank by rank (check_sorted), which is its exact image under a sort.
"""
from __future__ import annotations

import numpy as np

import sampling_numpy as sn

ULP = sn.ULP
NEAR, FAR = np.float32(0.02), np.float32(0.21)
MAX_LEFT_OUT = 0.02

# shape -> rays: 1, 5 and counts that are no multiple of 4 (four rays per block, one wave per ray)
SIGMA_CASES = {2: 1, 3: 5, 64: 22, 65: 22, 128: 23, 129: 22, 256: 64}                 # N edges -> B
PDF_CASES = {(1, 7): 1, (64, 64): 13, (65, 100): 5, (128, 256): 14, (129, 64): 22, (255, 300): 64}
GUIDED_CASES = {2: 1, 5: 13, 64: 22, 65: 23, 100: 14, 128: 64}                          # n -> B
STRAT_CASES = {2: (5, 8), 5: (1, 11), 64: (22, 11), 129: (63, 8)}                      # S -> (B, ray stride)

# The K oracle/ref_cpu.py needs (this module's __main__ prints them), rounded up to two digits.
K_ORACLE = {
    ("sigma", 2): 0,                  # measured 0; one bin: the CDF is 0, 1
    ("sigma", 3): 0,                  # measured 0; two equal bins: the CDF is 0, 0.5, 1
    ("sigma", 64): 1.4,               # measured 1.395; worst kept error 1.74e-07, left out 1.07% (a row: 3%)
    ("sigma", 65): 1.9,               # measured 1.817; 3.96e-07, 0.91% (3%)
    ("sigma", 128): 0.89,             # measured 0.8886; 1.03e-07, 0.41% (2%)
    ("sigma", 129): 1.5,              # measured 1.435; 2.11e-07, 0.46% (2%)
    ("sigma", 256): 1.7,              # measured 1.681; 3.33e-07, 0.18% (1%)
    ("pdf", 1, 7): 0,                 # measured 0; one bin
    ("pdf", 64, 64): 2,               # measured 1.98; 2.91e-05, 0.84% (3%)
    ("pdf", 65, 100): 0.91,           # measured 0.9079; 1.89e-07, 0.40% (2%)
    ("pdf", 128, 256): 1.9,           # measured 1.819; 5.47e-07, 0.25% (1%)
    ("pdf", 129, 64): 1.3,            # measured 1.288; 6.55e-06, 1.49% (5%)
    ("pdf", 255, 300): 2,             # measured 1.988; 1.11e-05, 0.34% (2%)
    ("guided", 2, "train"): 0,        # measured 0; one bin
    ("guided", 2, "test"): 0,
    ("guided", 5, "train"): 0.89,     # measured 0.8841; 4.32e-07, 0.00%
    ("guided", 5, "test"): 1.9,       # measured 1.854; 8.21e-07, 0.00%
    ("guided", 64, "train"): 1.8,     # measured 1.722; 8.98e-08, 0.64% (3%)
    ("guided", 64, "test"): 1.9,      # measured 1.885; 5.65e-07, 1.42% (3%)
    ("guided", 65, "train"): 1.6,     # measured 1.57; 1.95e-07, 0.80% (3%)
    ("guided", 65, "test"): 1.6,      # measured 1.57; 2.60e-07, 1.67% (3%)
    ("guided", 100, "train"): 0.9,    # measured 0.8939; 1.08e-07, 0.50% (2%)
    ("guided", 100, "test"): 1.9,     # measured 1.854; 4.92e-07, 0.86% (2%)
    ("guided", 128, "train"): 1.9,    # measured 1.899; 5.02e-07, 0.32% (2%)
    ("guided", 128, "test"): 1.9,     # measured 1.899; 5.02e-07, 0.85% (2%)
    ("guided_deg", 5): 0.89,          # degenerate_guided_case, its ordinary rays: measured 0.8841; 4.32e-07, 0.00%
    ("guided_deg", 64): 1.8,          # measured 1.722; 8.98e-08, 0.57% (3%)
    ("guided_deg", 65): 1.6,          # measured 1.57; 1.95e-07, 0.74% (3%)
    ("guided_deg", 128): 1.9,         # measured 1.819; 2.87e-07, 0.29% (2%)
}


def draws(g, B, n):
    """multiples of 2^-24 in [0, 1) like torch.rand's; column 0 is 0 and the last 1 - 2^-24"""
    u = (g.integers(0, 2 ** 24, (B, n)).astype(np.float64) * ULP).astype(np.float32)
    u[:, 0] = 0.0
    u[:, -1] = np.float32(1.0 - ULP)
    return u


def windows(g, B):
    """(centre, spread) rows: inside [NEAR, FAR], clamped on one side, on both, wholly outside,
    spreads from 1e-6 to 0.5; row 0 is an ordinary window (the one-ray cases)"""
    fixed = [(0.1, 0.01), (0.12, 1e-6), (0.11, 1e-4), (0.03, 0.02), (0.2, 0.02), (0.1, 0.5), (0.15, 0.1),
             (-0.1, 0.01), (0.4, 0.05), (0.021, 1e-3), (0.2099, 1e-5), (0.1, 0.0301)]
    c = np.array([f[0] for f in fixed] + list(g.uniform(0.0, 0.25, max(B - len(fixed), 0))))[:B]
    sd = np.array([f[1] for f in fixed] + list(10.0 ** g.uniform(-6.0, np.log10(0.5), max(B - len(fixed), 0))))[:B]
    return c.astype(np.float32), sd.astype(np.float32)


def sigma_case(N):
    B = SIGMA_CASES[N]
    g = np.random.default_rng(1000 + N)
    c, sd = windows(g, B)
    three = np.float32(3.0)
    return dict(low=c - three * sd, high=c + three * sd, n=N, near=NEAR, far=FAR, u=draws(g, B, N))


def weight_rows(g, B, nb):
    """all zeros / alternating zeros / one spike of weight 1 / smooth and normalised like compositing
    weights / uniform / uniform^4, cycled; row 0 is the smooth one"""
    w = np.zeros((B, nb), np.float32)
    k = np.arange(nb)
    for r in range(B):
        kind = r % 6
        if kind == 0:
            mu, s = g.uniform(0.2, 0.8) * nb, g.uniform(0.02, 0.2) * nb + 0.5
            v = np.exp(-0.5 * ((k - mu) / s) ** 2)
            w[r] = v / v.sum()
        elif kind == 1:
            pass
        elif kind == 2:
            w[r] = g.uniform(0.0, 1.0, nb) * (k % 2 == r // 6 % 2)
        elif kind == 3:
            w[r, g.integers(0, nb)] = 1.0
        elif kind == 4:
            w[r] = g.uniform(0.0, 1.0, nb)
        else:
            w[r] = g.uniform(0.0, 1.0, nb) ** 4
    return w


def pdf_case(nb, n_imp):
    B = PDF_CASES[(nb, n_imp)]
    g = np.random.default_rng(2000 + nb)
    bins = np.sort(g.uniform(NEAR, FAR, (B, nb + 1)), -1).astype(np.float32)
    return dict(bins=bins, w=weight_rows(g, B, nb), u=draws(g, B, n_imp))


def guided_case(n, train):
    """pass-1 depths and weights with the predicted window low in [NEAR, FAR] and the GT window
    high in it, far apart: taking the wrong window or the wrong row of draws misses by a wide margin"""
    B = GUIDED_CASES[n]
    g = np.random.default_rng(3000 + n)
    z = np.sort(g.uniform(NEAR, FAR, (B, n)), -1).astype(np.float32)
    w = np.zeros((B, n), np.float32)
    for r in range(B):
        kind = r % 4
        if kind == 3:                      # uniform weights: a window clamped on both sides
            v = np.ones(n)
        else:                              # a bump low on the ray, widths from a sample to a third of it
            mu, s = g.uniform(0.03, 0.09), 10.0 ** g.uniform(-3.0, -1.5)
            v = np.exp(-0.5 * ((z[r] - mu) / s) ** 2) + 1e-9
        w[r] = v / v.sum() * g.uniform(0.5, 1.0)
    depth = (w.astype(np.float64) * z).sum(-1).astype(np.float32)
    valid = (np.arange(B) % 3 != 1).astype(np.int64)
    gt = g.uniform(0.15, 0.19, B)
    gs = 10.0 ** g.uniform(-6.0, -2.0, B)
    for r, (c, s) in enumerate([(0.2, 0.02), (0.17, 0.2), (0.5, 0.01), (0.16, 1e-6)]):   # clamped one side / both / outside / tiny
        if 3 * r < B:
            gt[3 * r], gs[3 * r] = c, s
    tdep = np.stack([gt, np.ones(B)], 1).astype(np.float32)
    d = dict(z=z, depth=depth, w=w, nf=np.array([NEAR, FAR], np.float32), valid=valid if train else None,
             tdep=tdep, tstd=gs.astype(np.float32), u_pred=draws(g, B, n), u_gt=draws(g, B, n))
    return d


def strat_case(S):
    B, stride = STRAT_CASES[S]
    g = np.random.default_rng(4000 + S)
    rays = g.standard_normal((B, stride)).astype(np.float32)
    rays[:, 6] = g.uniform(0.0, 0.05, B)
    rays[:, 7] = rays[:, 6] + g.uniform(0.1, 0.3, B)
    rays[0, 7] = rays[0, 6]                       # near = far
    if B > 2:
        rays[2, 6], rays[2, 7] = -0.3, 0.4        # a range across zero
    return dict(rays=rays, u=draws(g, B, S), S=S)


def entry_case(nb):
    """all-zero weights over nb = 2^k bins: every (w + eps) / sum is 1 / nb and the CDF k / nb, exact in
    float32 in any order of summation.  Draw k / nb lies ON entry k and, by searchsorted(right=True),
    starts bin k with u - c = 0: the sample is b_k bit for bit.  (Searching with < in place of <=
    takes bin k - 1 and returns b_{k-1} + 1.0 * (b_k - b_{k-1}), another float32 for many edges.)"""
    assert nb & (nb - 1) == 0
    g = np.random.default_rng(5000 + nb)
    bins = g.uniform(-1.0, 1.0, (5, nb + 1)).astype(np.float32)     # unsorted, both signs: b_k - b_{k-1} rounds
    u = np.tile((np.arange(nb) / nb).astype(np.float32), (5, 1))
    return dict(bins=bins, w=np.zeros((5, nb), np.float32), u=u)


ZERO_WIDTH_N = (2, 8, 64, 65, 129, 256)


def zero_width_case(N):
    """sample_3sigma windows of zero width inside [NEAR, FAR], at either bound and outside; the last
    row's spread is a denormal: high != low, but the float32 step (high - low) / (N - 1) is 0"""
    low = np.array([0.1, 0.0, NEAR, FAR, -0.1, 0.3, 0.15, 0.1234567, 1e-3, 0.0], np.float32)
    high = low.copy()
    high[-1] = np.float32(1e-44)
    assert high[-1] > 0
    return dict(low=low, high=high, near=NEAR, far=FAR, u=draws(np.random.default_rng(N), len(low), N))


DEGENERATE_N = (5, 64, 65, 128)
DEGENERATE_ROWS = (0, 4, 1, 2, 5)


def degenerate_guided_case(n):
    """guided_case(n, train) with five zero-width windows among its rays: all of pass 1's weight on
    one sample (row 0 inside, row 4 on the first sample), an empty ray with depth 0 (row 1),
    target_std = 0 on a valid ray (row 2 inside, row 5 beyond far); the rest stay ordinary rays.
    d["centre"] is the window centre of DEGENERATE_ROWS, before the clamp."""
    d = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in guided_case(n, True).items()}
    assert d["z"].shape[0] > 7
    d["valid"][:7] = [0, 0, 1, 0, 0, 1, 0]
    for r, k in ((0, n // 2), (4, 0)):
        d["w"][r] = 0.0
        d["w"][r, k] = 1.0
        d["depth"][r] = d["z"][r, k]
    d["w"][1], d["depth"][1] = 0.0, 0.0
    d["tstd"][2], d["tdep"][2, 0] = 0.0, 0.17
    d["tstd"][5], d["tdep"][5, 0] = 0.0, 0.4
    d["centre"] = np.array([d["depth"][0], d["depth"][4], 0.0, 0.17, 0.4], np.float32)
    return d


def degenerate_mask(d):
    m = np.zeros(d["z"].shape[0], bool)
    m[list(DEGENERATE_ROWS)] = True
    return m


def rows(p: sn.Pdf, keep):
    """the Pdf of a subset of rays"""
    return sn.Pdf(p.s[keep], p.den[keep], p.bw[keep], p.amb[keep], p.lo[keep], p.hi[keep], p.edge_slope[keep], p.nb)


def guided_ref(d, detail=True):
    return sn.guided(d["z"], d["depth"], d["w"], d["nf"], d["valid"], d["tdep"][:, 0], d["tstd"], d["u_pred"], d["u_gt"],
                     detail=detail)


# ---- the bound -------------------------------------------------------------------------------

def k_needed(got, p: sn.Pdf):
    """The K a result needs on the kept draws of p; inf where a draw of zero slope misses 4 ulp."""
    err = np.abs(got.astype(np.float64) - p.s)
    rest = np.maximum(err - 4.0 * ULP * np.abs(p.s), 0.0)
    unit = ULP * np.abs(p.bw) / p.den
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(rest == 0.0, 0.0, rest / unit)
    k = np.where(p.amb, 0.0, k)
    return float(k.max()), float(np.where(p.amb, 0.0, err).max())


def left_out(p: sn.Pdf):
    """(share of the case, largest share of a row) the ambiguity mask excuses"""
    return float(p.amb.mean()), float(p.amb.mean(-1).max())


def check_cap(p: sn.Pdf, what=""):
    share, row = left_out(p)
    assert share <= MAX_LEFT_OUT, f"{what}: the ambiguity mask leaves out {share:.2%} of the case"
    assert row <= 0.5, f"{what}: the ambiguity mask leaves out {row:.0%} of a row"
    return share, row


def tol_of(p: sn.Pdf, K):
    return K * ULP * np.abs(p.bw) / p.den + 4.0 * ULP * np.abs(p.s)


def check_values(got, p: sn.Pdf, K, what=""):
    """kept draws within the bound; excused draws finite and inside their tiny bins' hull"""
    got = got.astype(np.float64)
    assert np.isfinite(got).all(), f"{what}: non-finite samples"
    err, tol = np.abs(got - p.s), tol_of(p, K)
    bad = ~p.amb & (err > tol)
    need, worst = k_needed(got, p)
    print(f"{what}: K needed {need:.3g} (bound {K:.3g}), worst kept error {worst:.3e}, left out {p.amb.mean():.2%}")
    assert not bad.any(), (f"{what}: {int(bad.sum())} samples miss the bound, first at {tuple(np.argwhere(bad)[0])}: "
                           f"error {err[bad].max():.3e}, K needed {need:.3g} > {K:.3g}")
    if p.amb.any():
        lo, hi = interval(p, K)
        a = p.amb
        inside = (got[a] >= lo[a]) & (got[a] <= hi[a])
        assert inside.all(), f"{what}: {int((~inside).sum())} excused samples leave their tiny bins"


def interval(p: sn.Pdf, K):
    """per draw, where a result may lie: [s - tol, s + tol], and for an excused draw its tiny bins'
    hull [lo, hi] widened by what a draw within delta = (nb + 2) 2^-24 of the hull's ends moves by on
    the steepest bin next to it, the bound's two terms on top"""
    tol = tol_of(p, K)
    slack = ((p.nb + 2) + K) * ULP * p.edge_slope + 4.0 * ULP * np.maximum(np.abs(p.s), np.nan_to_num(np.maximum(np.abs(p.lo), np.abs(p.hi))))
    lo = np.where(p.amb, np.nan_to_num(p.lo) - slack, p.s - tol)
    hi = np.where(p.amb, np.nan_to_num(p.hi) + slack, p.s + tol)
    return lo, hi


def check_sorted(got_sorted, p: sn.Pdf, K, what="", exact=None):
    """The per-draw bound under a sort: if lo_i <= x_i <= hi_i for every draw then, rank by rank,
    sort(lo) <= sort(x) <= sort(hi).  exact (B, m): values merged in as they are (z, in z_sorted)."""
    lo, hi = interval(p, K)
    if exact is not None:
        lo, hi = np.concatenate([exact, lo], -1), np.concatenate([exact, hi], -1)
    lo, hi = np.sort(lo, -1), np.sort(hi, -1)
    got = got_sorted.astype(np.float64)
    assert np.isfinite(got).all(), f"{what}: non-finite samples"
    over = np.maximum(np.maximum(lo - got, got - hi), 0.0)
    print(f"{what}: worst excess over the rank-wise bound {float(over.max()):.3e}, left out {p.amb.mean():.2%}")
    bad = over > 0
    assert not bad.any(), (f"{what}: {int(bad.sum())} sorted samples leave the rank-wise bound, first at "
                           f"{tuple(np.argwhere(bad)[0])}, by {float(over.max()):.3e}")


def oracle_k():
    """K of oracle/ref_cpu.py against the restatement, per shape (and the left-out shares)"""
    import torch
    from oracle import ref_cpu
    T = torch.tensor
    out = {}
    for N in SIGMA_CASES:
        d = sigma_case(N)
        got = ref_cpu.sample_3sigma(T(d["low"]), T(d["high"]), N, T(d["near"]), T(d["far"]), T(d["u"])).numpy()
        p = sn.sample_3sigma(d["low"], d["high"], N, d["near"], d["far"], d["u"])
        out[("sigma", N)] = k_needed(got, p) + left_out(p)
    for nb, n_imp in PDF_CASES:
        d = pdf_case(nb, n_imp)
        got = ref_cpu.sample_pdf(T(d["bins"]), T(d["w"]), T(d["u"])).numpy()
        p = sn.sample_pdf(d["bins"], d["w"], d["u"])
        out[("pdf", nb, n_imp)] = k_needed(got, p) + left_out(p)
    for n in GUIDED_CASES:
        for train in (True, False):
            d = guided_case(n, train)
            got = oracle_guided(d)
            p = guided_ref(d)[2]
            out[("guided", n, "train" if train else "test")] = k_needed(got, p) + left_out(p)
    for n in DEGENERATE_N:
        d = degenerate_guided_case(n)
        p = guided_ref(d)[2]
        keep = ~degenerate_mask(d)
        out[("guided_deg", n)] = k_needed(oracle_guided(d)[keep], rows(p, keep)) + left_out(p)
    return out


def oracle_guided(d):
    """the oracle's unsorted guided depths (ref_cpu.guided_depths), its GT draws the valid rows of u_gt"""
    import torch
    from oracle import ref_cpu
    T = torch.tensor
    train = d["valid"] is not None
    seq = [T(d["u_pred"])] + ([T(d["u_gt"][d["valid"] > 0])] if train else [])
    z2 = ref_cpu.guided_depths({"depth": T(d["depth"]), "weights": T(d["w"])}, T(d["z"]), d["z"].shape[1], T(d["nf"][0]),
                               T(d["nf"][1]), lambda kind, shape: seq.pop(0), train,
                               T(d["valid"]) if train else None, T(d["tdep"]), T(d["tstd"]))
    return z2.numpy()


if __name__ == "__main__":
    import math
    for key, (k, worst, share, row) in oracle_k().items():
        up = 0.0 if k == 0 else math.ceil(k / 10 ** (math.floor(math.log10(k)) - 1)) * 10 ** (math.floor(math.log10(k)) - 1)
        print(f"    {key!r}: {up:.2g},   # measured {k:.4g}; worst kept error {worst:.2e}, left out {share:.2%} (a row: {row:.0%})")
