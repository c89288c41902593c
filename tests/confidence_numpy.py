"""The numpy statement of the confidence planes (include/staged/spnerf_amd_confidence.h): written from the header
and apart from the kernel, with plain loops over the planes — every cell of a plane goes through each numpy
operation together — float32 where the header says fp32 and float64 where it says fp64.  ``sparsification`` is
the instrument's statement, a loop over the removed shares.
"""
import numpy as np

F = np.float32
D = np.float64
PLANES = ("scored", "index", "margin", "peak_margin", "peaks", "support", "curvature", "mlm", "spread")


def confidence(volume, step, tau, temperature, exclude=1):
    """dict of the nine planes, each (cells,) or the volume's trailing shape; ``volume`` (K, ...) float32."""
    v = np.asarray(volume, F)
    K, shape = v.shape[0], v.shape[1:]
    v = v.reshape(K, -1)
    n = v.shape[1]
    ok = np.isfinite(v)                                                   # scored
    tau, temperature, step = D(F(tau)), D(F(temperature)), D(step)
    nan = np.full(n, np.nan, F)

    scored = np.zeros(n, np.int32)
    index = np.full(n, -1, np.int32)
    best = nan.copy()
    for k in range(K):                                                    # the lowest plane holding the largest scored value
        scored += ok[k]
        take = ok[k] & ((index < 0) | (np.where(ok[k], v[k], 0).astype(D) > np.where(index >= 0, best, 0).astype(D)))
        index[take], best[take] = k, v[k][take]
    has = index >= 0
    best64 = best.astype(D)

    def at(k):                                                            # (values, scored) of plane k, nothing outside
        return (v[k], ok[k]) if 0 <= k < K else (nan, np.zeros(n, bool))

    second, other = nan.copy(), nan.copy()
    peaks, support = np.zeros(n, np.int32), np.zeros(n, np.int32)
    Z = np.zeros(n, D)
    with np.errstate(invalid="ignore", over="ignore"):
        floor = best64 - tau
        for k in range(K):
            s, on = at(k)
            on = on & has
            far = on & (np.abs(k - index) > exclude)
            up = far & (np.isnan(second) | (s > second))
            second[up] = s[up]
            (lo, lo_on), (hi, hi_on) = at(k - 1), at(k + 1)
            peak = on & (~lo_on | (s > lo)) & (~hi_on | (s >= hi))
            rival = peak & (k != index)
            up = rival & (np.isnan(other) | (s > other))
            other[up] = s[up]
            near = on & (s.astype(D) >= floor)
            peaks += peak & near
            support += near
            e = np.exp((np.where(on, s, 0).astype(D) - np.where(on, best64, 0)) / temperature)
            Z += np.where(on, e, 0.0)
        mlm = np.where(has, 1.0 / np.where(has, Z, 1.0), np.nan)
        V = np.zeros(n, D)
        for k in range(K):                                                # p_k = e_k · mlm, the second moment about the pick
            s, on = at(k)
            on = on & has
            e = np.exp((np.where(on, s, 0).astype(D) - np.where(on, best64, 0)) / temperature)
            V += np.where(on, e * mlm * (D(k) - index.astype(D)) ** 2, 0.0)
        spread = np.where(has, step * np.sqrt(V), np.nan)
        margin = np.where(np.isnan(second), F(np.nan), best - second).astype(F)
        peak_margin = np.where(np.isnan(other), F(np.nan), best - other).astype(F)

        below = np.full(n, np.nan, F)
        above = np.full(n, np.nan, F)
        for k in range(K):
            below[index == k + 1] = np.where(ok[k], v[k], F(np.nan))[index == k + 1]
            above[index == k - 1] = np.where(ok[k], v[k], F(np.nan))[index == k - 1]
        curvature = (-((below.astype(D) - 2.0 * best64) + above.astype(D))).astype(F)
    out = {"scored": scored, "index": index, "margin": margin, "peak_margin": peak_margin, "peaks": peaks, "support": support,
           "curvature": curvature, "mlm": mlm.astype(F), "spread": spread.astype(F)}
    for name in ("margin", "peak_margin", "curvature", "mlm", "spread"):  # one NaN: the quiet one
        out[name] = np.where(np.isnan(out[name]), F(np.nan), out[name]).astype(F)
    out["mlm64"], out["spread64"] = mlm, spread                           # before the cast, for the tolerances
    return {k: a.reshape(shape) for k, a in out.items()}


def sparsification(error, confidence, steps=100):
    """(curve (steps,) float64, area): the cells with both finite sorted by descending confidence, ties by cell
    index; the mean error of the n − ⌊n·i / steps⌋ cells kept; the trapezoid rule over i / steps, over curve[0]."""
    err, conf = np.asarray(error, D).ravel(), np.asarray(confidence, D).ravel()
    both = np.isfinite(err) & np.isfinite(conf)
    err, conf = err[both], conf[both]
    n = err.size
    order = sorted(range(n), key=lambda c: (-conf[c], c))
    err = err[order]
    curve = np.array([err[:n - (n * i) // steps].mean() for i in range(steps)])
    area = sum((curve[i] + curve[i + 1]) / 2 / steps for i in range(steps - 1)) / curve[0]
    return curve, float(area)
