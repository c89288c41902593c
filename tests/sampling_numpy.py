"""float64 numpy restatement of the depth samplers of the render path (the reference's
modules/rendering.py: stratified depths :131-144, ``sample_pdf`` :14-55, ``sample_3sigma`` :58-73,
``GenerateGuidedSamples`` :92-116 with the sort and cat of :165-167), as include/spnerf_amd.h
states them.  Every draw is an argument.

All arithmetic is float64 on the float32 inputs, but for the two roundings that belong to the
operation's definition:
  * ``w + eps`` is added in float32 (the weights the CDF is built from are float32 numbers);
  * the 3-sigma window's edges are rounded to float32 after the clamp: they are the ``bins`` the
    interpolation reads.
``eps`` itself is the float32 nearest to 1e-5, in the sum and in the ``den < eps`` rule.

sample_pdf, for bins b_0..b_nb, weights w_0..w_{nb-1} and a draw u in [0, 1):
  p_k = (w_k + eps) / sum_j (w_j + eps);  c_0 = 0, c_{k+1} = c_k + p_k;
  i = #{k : c_k <= u} (searchsorted, right = True), below = max(i - 1, 0), above = min(i, nb);
  den = c_above - c_below, replaced by 1 where den < eps;
  sample = b_below + (u - c_below) / den * (b_above - b_below).

The replacement makes the inverse CDF discontinuous: every draw inside a bin of mass below eps maps
to about b_k while the next bin starts at b_{k+1}.  Two correct float32 implementations may
therefore differ by a whole bin width when u lies within the CDF's rounding error of such a bin, or
when the bin's mass lies within rounding error of eps.  ``Pdf.amb`` marks exactly those draws:
u in [c_k - delta, c_{k+1} + delta] for any bin k of float64 mass below 1.1 eps, delta =
(nb + 2) 2^-24; ``Pdf.lo`` / ``Pdf.hi`` are the hull [min b_k, max b_{k+1}] over the bins that mark
the draw, and ``Pdf.edge_slope`` the largest bw / den among the selected bin and the two bins next to
that hull (what a draw within delta of the hull's ends can move by, per unit of u).

The library differs from the reference in one place, on purpose: a window of zero width
(the float32 step (high - low) / (n - 1) is 0; the reference divides 0 by 0 there and returns NaN)
gives n copies of the clamped window centre.  ``sample_3sigma`` and ``guided`` restate the library."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

ULP = 2.0 ** -24
EPS = 1e-5


@dataclass
class Pdf:
    s: np.ndarray            # (B, n) float64 samples
    den: np.ndarray          # (B, n) CDF mass of the selected bin, after den < eps -> 1
    bw: np.ndarray           # (B, n) b_above - b_below
    amb: np.ndarray          # (B, n) bool: the ambiguity mask
    lo: np.ndarray           # (B, n) hull of the tiny bins that mark the draw (NaN where amb is False)
    hi: np.ndarray
    edge_slope: np.ndarray   # (B, n) see the module docstring
    nb: int = 0              # the number of bins


def stratified(rays: np.ndarray, n: int, u: np.ndarray) -> np.ndarray:
    near, far = rays[:, 6:7].astype(np.float64), rays[:, 7:8].astype(np.float64)
    t = np.linspace(0.0, 1.0, n)
    z = near * (1.0 - t) + far * t
    mid = 0.5 * (z[:, :-1] + z[:, 1:])
    hi = np.concatenate([mid, z[:, -1:]], -1)
    lo = np.concatenate([z[:, :1], mid], -1)
    return lo + (hi - lo) * u.astype(np.float64)


def sample_pdf(bins: np.ndarray, w: np.ndarray, u: np.ndarray, eps: float = EPS) -> Pdf:
    assert bins.dtype == np.float32 and w.dtype == np.float32 and u.dtype == np.float32
    B, nb = w.shape
    n = u.shape[1]
    eps32 = np.float32(eps)
    e = float(eps32)
    we = (w + eps32).astype(np.float64)                     # the float32 sum, then float64
    p = we / we.sum(-1, keepdims=True)
    c = np.concatenate([np.zeros((B, 1)), np.cumsum(p, -1)], -1)
    b = bins.astype(np.float64)
    u64 = u.astype(np.float64)
    idx = np.stack([np.searchsorted(c[r], u64[r], side="right") for r in range(B)])
    below, above = np.maximum(idx - 1, 0), np.minimum(idx, nb)
    take = lambda a, i: np.take_along_axis(a, i, 1)
    c0, c1, b0, b1 = take(c, below), take(c, above), take(b, below), take(b, above)
    den = c1 - c0
    den = np.where(den < e, 1.0, den)
    bw = b1 - b0
    s = b0 + (u64 - c0) / den * bw

    # the ambiguity mask and what goes with it
    mass = c[:, 1:] - c[:, :-1]
    tiny = mass < 1.1 * e                                    # (B, nb)
    delta = (nb + 2) * ULP
    slope = np.abs(b[:, 1:] - b[:, :-1]) / np.where(mass < e, 1.0, mass)
    amb = np.zeros((B, n), bool)
    lo, hi = np.full((B, n), np.nan), np.full((B, n), np.nan)
    kmin, kmax = np.minimum(below, nb - 1), np.minimum(below, nb - 1)
    for r in range(B):
        ks = np.nonzero(tiny[r])[0]
        if ks.size == 0:
            continue
        hit = (u64[r][:, None] >= c[r, ks][None] - delta) & (u64[r][:, None] <= c[r, ks + 1][None] + delta)   # (n, tiny)
        amb[r] = hit.any(1)
        blo, bhi = np.minimum(b[r, ks], b[r, ks + 1]), np.maximum(b[r, ks], b[r, ks + 1])
        lo[r] = np.where(amb[r], np.where(hit, blo[None], np.inf).min(1), np.nan)
        hi[r] = np.where(amb[r], np.where(hit, bhi[None], -np.inf).max(1), np.nan)
        kmin[r] = np.where(amb[r], np.minimum(kmin[r], np.where(hit, ks[None], nb).min(1)), kmin[r])
        kmax[r] = np.where(amb[r], np.maximum(kmax[r], np.where(hit, ks[None], -1).max(1)), kmax[r])
    edge_slope = np.maximum(np.maximum(take(slope, np.maximum(kmin - 1, 0)), take(slope, np.minimum(kmax + 1, nb - 1))),
                            np.abs(bw) / den)
    return Pdf(s, den, bw, amb, lo, hi, edge_slope, nb)


def flat_window(low: np.ndarray, high: np.ndarray, n: int) -> np.ndarray:
    """(B, 1) bool: the float32 step (high - low) / (n - 1) is zero — low == high as float32 numbers,
    or a spread so small that the step underflows"""
    with np.errstate(under="ignore"):
        step = (high.astype(np.float32) - low.astype(np.float32)) / np.float32(n - 1)
    return (step == 0.0)[:, None]


def window_edges(low: np.ndarray, high: np.ndarray, n: int, near: float, far: float) -> np.ndarray:
    """The float32 bin edges of sample_3sigma; a zero-width window's are its clamped low end."""
    lo64, hi64 = low.astype(np.float64)[:, None], high.astype(np.float64)[:, None]
    t = np.linspace(0.0, 1.0, n)
    edges = np.where(flat_window(low, high, n), lo64 + 0.0 * t, lo64 * (1.0 - t) + hi64 * t)
    return np.clip(edges, float(near), float(far)).astype(np.float32)


def sample_3sigma(low: np.ndarray, high: np.ndarray, n: int, near: float, far: float, u: np.ndarray) -> Pdf:
    edges = window_edges(low, high, n, near, far)
    step = (high.astype(np.float64) - low.astype(np.float64))[:, None] / (n - 1)
    e64 = edges.astype(np.float64)
    flat = flat_window(low, high, n)
    factor = np.where(flat, 0.0, (e64[:, 1:] - e64[:, :-1]) / np.where(flat, 1.0, step))
    x = np.linspace(-3.0, 3.0, n - 1)
    gauss = 1.0 / np.sqrt(2.0 * np.pi) * np.exp(-0.5 * x * x)
    return sample_pdf(edges, (factor * gauss[None]).astype(np.float32), u)


def guided(z, depth, weights, clamp_nf, valid, tdepth, tstd, u_pred, u_gt, detail: bool = False):
    """(z_sorted, z_unsort) of spnerf_sample_guided: z_unsort = [z, sort(z2)], z_sorted = sort(z_unsort).
    valid None = test mode.  tdepth is the depth column (n_rays,), u_gt has one row per ray.
    detail = True adds the Pdf of the unsorted guided samples z2."""
    n = z.shape[1]
    z64, d64 = z.astype(np.float64), depth.astype(np.float64)
    std = np.sqrt((((z64 - d64[:, None]) ** 2) * weights.astype(np.float64)).sum(-1))
    low, high, u = d64 - 3.0 * std, d64 + 3.0 * std, u_pred
    if valid is not None:
        sel = np.asarray(valid) > 0
        gt, gs = tdepth.astype(np.float64), tstd.astype(np.float64)
        low, high = np.where(sel, gt - 3.0 * gs, low), np.where(sel, gt + 3.0 * gs, high)
        u = np.where(sel[:, None], u_gt, u_pred)
    p = sample_3sigma(low, high, n, clamp_nf[0], clamp_nf[1], u)
    z_unsort = np.concatenate([z64, np.sort(p.s, -1)], -1)
    z_sorted = np.sort(z_unsort, -1)
    return (z_sorted, z_unsort, p) if detail else (z_sorted, z_unsort)
