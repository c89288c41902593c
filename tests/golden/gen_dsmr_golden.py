"""Generate tests/golden/dsmr.npz by running the REFERENCE's DSM registration (modules/dsmr.py)
on crops of the lidar truth already in dsm_truth.npz.  CPU only, a few minutes:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_dsmr_golden.py [--ref /root/reference]

numba and rasterio are not installed, so two stub modules stand in for them before the import:
``numba.jit`` is an identity decorator (the loops run as plain Python, in float64 on float64
input like numba's accumulators) and ``rasterio`` is empty (only ``readimg`` uses it, and this
script never calls ``readimg``).  Only data is stored.  Per case ``c`` in a, b, c:

    c_u, c_v            float32 (H, W): the reference DSM and the DSM to register, as read from TIFFs
    c_shifts            int64 (levels, 2): (dx, dy) recursive_ncc returns at every level, finest first
    c_tables            float64 (levels, 2r+1, 2r+1): ncc of every shift of every level (rows y),
                        NaN where no finite pair overlaps (pure Python divides by zero there)
    c_moments           float64 (6,): mean_std at the result (muu, muv, sigu, sigv, xcorr) and the pair count
    c_down              float64: downsample2x(u)
    c_shift_scaled / c_shift_plain   float64 (4,): (dx, dy, a, b) with scaling=True / False
    c_applied           float32 (H, W): apply_shift_ of float32 v with the scaling=False transform
    c_mae               float64: nanmean |applied - u| in the reference's float32 arithmetic

``--dry`` evaluates the cases with the numpy restatement (tests/dsmr_numpy.py) instead of the
reference — seconds instead of minutes — to choose crops and seeds; it writes nothing.
"""
from __future__ import annotations

import argparse
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
IRANGE = 5
MIN_GAP = 1e-6


def load_reference(ref: str):
    numba = types.ModuleType("numba")
    numba.jit = lambda f=None, *a, **k: f if callable(f) else (lambda g: g)
    sys.modules.setdefault("numba", numba)
    sys.modules.setdefault("rasterio", types.ModuleType("rasterio"))
    sys.path.insert(0, ref)
    sys.dont_write_bytecode = True
    import modules.dsmr as dsmr  # noqa
    return dsmr


def crop_pair(gt, h, w, y0, x0, dx, dy):
    """u = gt[y0:, x0:] and v cut so that u[j, i] = v[j + dy, i + dx]."""
    u = gt[y0:y0 + h, x0:x0 + w].astype(np.float64)
    v = gt[y0 - dy:y0 - dy + h, x0 - dx:x0 - dx + w].astype(np.float64)
    assert u.shape == (h, w) and v.shape == (h, w)
    return u, v


def cases(gt):
    out = {}
    # (a) 136 x 120, two levels, true shift (+7, -4)
    rng = np.random.default_rng(3)
    u, v = crop_pair(gt, 136, 120, 200, 180, 7, -4)
    v = v + 2.5 + 0.05 * rng.standard_normal(v.shape)
    v[rng.random(v.shape) < 0.10] = np.nan
    u[rng.random(u.shape) < 0.03] = np.nan
    v[60:80, 40:70] = np.nan
    out["a"] = (u, v, (7, -4))
    # (b) 217 x 205, three levels (109 x 103, 55 x 52), odd sizes at two of them; the true shift
    # is negative and odd in x, so dx // 2 floors a negative number on the way down
    rng = np.random.default_rng(11)
    u, v = crop_pair(gt, 217, 205, 150, 140, -9, 6)
    v = v - 1.25 + 0.05 * rng.standard_normal(v.shape)
    v[rng.random(v.shape) < 0.05] = np.nan
    u[rng.random(u.shape) < 0.02] = np.nan
    u[100:125, 10:30] = np.nan
    out["b"] = (u, v, (-9, 6))
    # (c) 37 x 53, one level; u is finite in its first 12 columns only and v from column 8 on, so
    # no pixel pairs up at the shifts with x <= -4
    rng = np.random.default_rng(5)
    u, v = crop_pair(gt, 37, 53, 300, 260, 2, -1)
    v = v + 0.75 + 0.02 * rng.standard_normal(v.shape)
    u[:, 12:] = np.nan
    v[:, :8] = np.nan
    v[rng.random(v.shape) < 0.05] = np.nan
    out["c"] = (u, v, (2, -1))
    return {k: (a.astype(np.float32), b.astype(np.float32), s) for k, (a, b, s) in out.items()}


def check_gaps(name, tables, moments):
    """The condition the tests rest on: at every level the best finite ncc beats the runner-up
    by MIN_GAP, so the argmax is far from rounding; and both deviations are positive."""
    for lv, t in enumerate(tables):
        f = np.sort(t[np.isfinite(t)])
        assert f.size >= 2, (name, lv, "fewer than two finite correlations")
        gap = f[-1] - f[-2]
        print(f"  case {name} level {lv}: best {f[-1]:.6f}, gap to the runner-up {gap:.3e}, "
              f"{int(np.isnan(t).sum())} shifts without a pair")
        assert gap >= MIN_GAP, (name, lv, gap)
    assert moments[2] > 0 and moments[3] > 0, (name, moments)


def run_reference(dsmr, u32, v32):
    u, v = u32.astype(np.float64)[None], v32.astype(np.float64)[None]
    tables, shifts, cur = [], [], []
    ncc0, compute0 = dsmr.ncc, dsmr.compute_ncc

    def ncc(a, b, dx=0, dy=0):
        try:
            with np.errstate(invalid="ignore", divide="ignore"):
                c = float(ncc0(a, b, dx, dy))
        except ZeroDivisionError:       # no finite pair: numba's 0 / 0
            c = float("nan")
        cur.append(c)
        return c

    def compute_ncc(a, b, irange, initdx, initdy):
        cur.clear()
        d = compute0(a, b, irange, initdx, initdy)
        tables.append(np.array(cur).reshape(2 * irange + 1, 2 * irange + 1))
        shifts.append(d)
        return d

    dsmr.ncc, dsmr.compute_ncc = ncc, compute_ncc
    try:
        dx, dy = dsmr.recursive_ncc(u, v, IRANGE)
    finally:
        dsmr.ncc, dsmr.compute_ncc = ncc0, compute0
    m = dsmr.mean_std(u, v, dx, dy)
    res = {}
    for key, scaling in (("shift_scaled", True), ("shift_plain", False)):
        # compute_shift's last lines (readimg, its first, needs rasterio)
        a = m[2] / m[3] if scaling else 1
        res[key] = (dx, dy, a, m[0] - m[1] * a)
    v1 = v32[None]
    applied = dsmr.apply_shift_(v1, np.zeros_like(v1), res["shift_plain"][0], res["shift_plain"][1],
                                res["shift_plain"][2], res["shift_plain"][3], 0, 0)[0]
    return (shifts[::-1], tables[::-1], m, dsmr.downsample2x(u)[0], res, applied)


def run_numpy(u32, v32):
    sys.path.insert(0, os.path.dirname(HERE))
    import dsmr_numpy as dn
    trace = []
    dx, dy, _, _, m = dn.compute_shift(u32, v32, True, IRANGE, trace=trace)
    return [(t[0], t[1]) for t in trace[::-1]], [t[2] for t in trace[::-1]], m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--dry", action="store_true")
    ap.add_argument("--out", default=os.path.join(HERE, "dsmr.npz"))
    args = ap.parse_args()
    gt = np.load(os.path.join(HERE, "dsm_truth.npz"))["gt"]
    dsmr = None if args.dry else load_reference(args.ref)
    store = {}
    for name, (u, v, true_shift) in cases(gt).items():
        print(f"case {name}: {u.shape[0]} x {u.shape[1]}, true shift {true_shift}", flush=True)
        if args.dry:
            shifts, tables, m = run_numpy(u, v)
            check_gaps(name, tables, m)
            print("  shifts", shifts)
            assert tuple(shifts[0]) == true_shift
            continue
        shifts, tables, m, down, res, applied = run_reference(dsmr, u, v)
        count = int((np.isfinite(u) & np.isfinite(applied)).sum())     # mean_std's count at the result
        check_gaps(name, tables, m)
        assert tuple(shifts[0]) == true_shift, (shifts, true_shift)
        with np.errstate(invalid="ignore"):
            mae = np.nanmean(abs((applied - u).ravel()))
        print(f"  shifts {shifts}, a,b scaled {res['shift_scaled'][2:]}, plain {res['shift_plain'][2:]}, MAE {mae}")
        store[f"{name}_u"], store[f"{name}_v"] = u, v
        store[f"{name}_shifts"] = np.array(shifts, np.int64)
        store[f"{name}_tables"] = np.array(tables, np.float64)
        store[f"{name}_moments"] = np.array(list(m) + [count], np.float64)
        store[f"{name}_down"] = np.asarray(down, np.float64)
        store[f"{name}_shift_scaled"] = np.array(res["shift_scaled"], np.float64)
        store[f"{name}_shift_plain"] = np.array(res["shift_plain"], np.float64)
        assert applied.dtype == np.float32
        store[f"{name}_applied"] = applied
        store[f"{name}_mae"] = np.float64(mae)
    if not args.dry:
        np.savez_compressed(args.out, **store)
        print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
