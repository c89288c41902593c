"""The fp64 numpy statement of the geometric shadows (include/spnerf_amd_shadow.h): a ground-grid DSM
cast under K sun directions, and the agreement of a learnt sun plane with the result.  No early exit:
every cell marches to the grid's edge.  ``cast`` states the definition one step at a time for the
whole grid; ``cast_cell`` states it again with plain loops for one cell (tests/test_shadow_ref.py
holds the two together and pins them to known answers).

Every product and sum below is one numpy operation, i.e. rounded once: the kernel is compiled
without fused multiply-adds so that floor(y) cannot flip against this statement.
"""
import numpy as np


def march(direction, resolution):
    """(axis, sgn, q, rho) of a direction (east, north, up): axis 0 steps along the columns, 1 along
    the rows, None takes no step.  The direction is rounded to float32 first, as the library takes it."""
    e, n, u = (np.float64(v) for v in np.asarray(direction, np.float32))
    a, b = e, -n
    if a == 0.0 and b == 0.0:
        return None, 0, np.float64(0.0), np.float64(0.0)
    if abs(a) >= abs(b):
        return 0, (1 if a > 0 else -1), b / abs(a), np.float64(resolution) * u / abs(a)
    return 1, (1 if b > 0 else -1), a / abs(b), np.float64(resolution) * u / abs(b)


def _interp(h0, h1, f):
    """The height between two cell centres: linear, kept within its two heights; NaN if either is."""
    t = h0 + f * (h1 - h0)
    return np.minimum(np.maximum(t, np.minimum(h0, h1)), np.maximum(h0, h1))


def cast_one(dsm, resolution, direction):
    """(shadow uint8, excess float64) of one direction, both (H, W)."""
    dsm = np.asarray(dsm, np.float64)
    axis, sgn, q, rho = march(direction, resolution)
    h = dsm.T if axis == 1 else dsm        # the row case is the transpose of the column case
    H, W = h.shape
    excess = np.full((H, W), -np.inf)
    if axis is not None:
        jj = np.arange(H, dtype=np.float64)
        ii = np.arange(W)
        with np.errstate(invalid="ignore"):
            for m in range(1, W):
                cols = ii + m * sgn
                okc = (cols >= 0) & (cols < W)
                y = jj + np.float64(m) * q
                okr = (y >= 0.0) & (y <= H - 1.0)
                if not okc.any() or not okr.any():
                    break                                    # y is monotone in m: it has left for good
                fl = np.floor(y)
                f = y - fl
                r0 = np.clip(fl.astype(np.int64), 0, H - 1)
                r1 = np.clip(r0 + 1, 0, H - 1)
                cc = np.clip(cols, 0, W - 1)
                h0, h1 = h[r0[:, None], cc[None, :]], h[r1[:, None], cc[None, :]]
                hs = np.where(f[:, None] == 0.0, h0, _interp(h0, h1, f[:, None]))
                e = (hs - h) - np.float64(m) * rho
                ok = okr[:, None] & okc[None, :] & ~np.isnan(hs) & ~np.isnan(h)
                excess = np.where(ok, np.maximum(excess, np.where(ok, e, -np.inf)), excess)
    with np.errstate(invalid="ignore"):
        shadow = np.where(excess > 0.0, 1, 0).astype(np.uint8)
    shadow[np.isnan(h)] = 255
    excess[np.isnan(h)] = np.nan
    return (shadow.T, excess.T) if axis == 1 else (shadow, excess)


def cast(dsm, resolution, dirs):
    """shadow (K, H, W) uint8 and excess (K, H, W) float64."""
    res = [cast_one(dsm, resolution, d) for d in np.asarray(dirs).reshape(-1, 3)]
    return np.stack([s for s, _ in res]), np.stack([e for _, e in res])


def cast_cell(dsm, resolution, direction, j, i):
    """(shadow, excess) of cell (j, i) under one direction, with plain loops."""
    dsm = np.asarray(dsm, np.float64)
    H, W = dsm.shape
    h = dsm[j, i]
    if np.isnan(h):
        return 255, np.nan
    axis, sgn, q, rho = march(direction, resolution)
    excess = -np.inf
    m = 0
    while axis is not None:
        m += 1
        if axis == 0:
            c, y, last = i + m * sgn, np.float64(j) + np.float64(m) * q, H - 1
            inside = 0 <= c < W
        else:
            c, y, last = j + m * sgn, np.float64(i) + np.float64(m) * q, W - 1
            inside = 0 <= c < H
        if not inside or not 0.0 <= y <= last:
            break
        r = int(np.floor(y))
        f = y - np.floor(y)
        at = (lambda k: dsm[k, c]) if axis == 0 else (lambda k: dsm[c, k])
        hs = at(r) if f == 0.0 else _interp(at(r), at(r + 1), f)
        if np.isnan(hs):
            continue
        excess = max(excess, (hs - h) - np.float64(m) * rho)
    return (1 if excess > 0.0 else 0), excess


def tolerance(dsm):
    """What the device's ``excess`` may differ by: 64·2⁻⁵²·max(1, max|h|)·max(H, W) metres — the
    rounding of y = j + m·q times the largest height difference."""
    dsm = np.asarray(dsm, np.float64)
    top = np.nanmax(np.abs(dsm)) if np.isfinite(dsm).any() else 0.0
    return 64.0 * 2.0 ** -52 * max(1.0, float(top)) * max(dsm.shape)


def agreement_sums(sun, shadow):
    """The per-direction sums and counts of spnerf_shadow_agreement_result, as a dict of length-K arrays."""
    sun, shadow = np.asarray(sun, np.float32), np.asarray(shadow, np.uint8)
    K = sun.shape[0]
    out = {k: np.zeros(K, np.float64) for k in ("sum_sun_lit", "sum_sun_shadow", "sum_abs")}
    out.update({k: np.zeros(K, np.int64) for k in ("n_lit", "n_shadow", "tp", "fp", "fn")})
    for k in range(K):
        s, v = shadow[k].reshape(-1), sun[k].reshape(-1).astype(np.float64)
        ok = (s <= 1) & np.isfinite(v)
        s, v = s[ok].astype(np.int64), v[ok]
        dark = v < 0.5
        out["n_lit"][k], out["n_shadow"][k] = int((s == 0).sum()), int((s == 1).sum())
        out["sum_sun_lit"][k], out["sum_sun_shadow"][k] = v[s == 0].sum(), v[s == 1].sum()
        out["sum_abs"][k] = np.abs(v - (1 - s)).sum()
        out["tp"][k], out["fp"][k], out["fn"][k] = int(((s == 1) & dark).sum()), int(((s == 0) & dark).sum()), int(((s == 1) & ~dark).sum())
    return out


def agreement(sun, shadow):
    """``shadow_agreement``'s dictionary: n, mae, mean_sun_lit, mean_sun_shadow, iou (NaN where a
    denominator is 0)."""
    t = agreement_sums(sun, shadow)

    def ratio(a, b):
        return np.array([x / y if y else np.nan for x, y in zip(np.asarray(a, np.float64), np.asarray(b, np.float64))])

    n = t["n_lit"] + t["n_shadow"]
    return {"n": n, "mae": ratio(t["sum_abs"], n), "mean_sun_lit": ratio(t["sum_sun_lit"], t["n_lit"]),
            "mean_sun_shadow": ratio(t["sum_sun_shadow"], t["n_shadow"]), "iou": ratio(t["tp"], t["tp"] + t["fp"] + t["fn"])}
