"""The depth samplers (csrc/sampling.hip: k_stratified, k_sample_pdf<1|2|4> also in sample_3sigma
mode, k_guided<1|2>) against the float64 restatement tests/sampling_numpy.py, at sizes on both sides
of every lane-layout switch — needs an MI355X.

Sizes: 64 | 65 edges (one | two elements per lane), 128 | 129 (two | four), 256 (the upper end);
n_samples 64 | 65 for k_guided<1> | k_guided<2>; n = 5, 65, 100 pad both bitonic sorts.  Inputs,
bound and constants are those of tests/sampling_cases.py (vetted on the CPU by
tests/test_sampling_ref.py); draws are passed explicitly (tests/test_gpu_philox.py ties the device
draws to this path bit for bit).  Each kernel gets twice the K the float32 oracle needs
(sampling_cases.K_ORACLE); every test prints the K its kernel needed.
"""
import numpy as np
import pytest
import torch

import sampling_cases as sc
import sampling_numpy as sn
from spnerf_amd import _lib
from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu

SENTINEL = -77.0


def dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV).contiguous()


def out_rows(B, n):
    """B rows to write and one more that must keep its sentinel"""
    return torch.full((B + 1, n), SENTINEL, device=DEV)


def rows_of(t, B):
    a = t.cpu().numpy()
    assert (a[B] == np.float32(SENTINEL)).all(), "the kernel wrote past row B"
    return a[:B]


def run_3sigma(d):
    B, N = d["u"].shape
    out = out_rows(B, N)
    low, high, nf, u = dev(d["low"]), dev(d["high"]), dev(np.array([d["near"], d["far"]], np.float32)), dev(d["u"])
    _lib.check(_lib.lib().spnerf_sample_3sigma(B, N, _lib.ptr(low), _lib.ptr(high), _lib.ptr(nf), _lib.ptr(u), _lib.ptr(out),
                                               _lib.stream_of(out)), "sample_3sigma")
    return rows_of(out, B)


def run_guided(d):
    B, n = d["z"].shape
    zs, zu = out_rows(B, 2 * n), out_rows(B, 2 * n)
    t = {k: dev(d[k]) for k in ("z", "depth", "w", "nf", "tdep", "tstd", "u_pred", "u_gt")}
    train = d["valid"] is not None
    valid = dev(d["valid"], torch.int64) if train else None
    _lib.check(_lib.lib().spnerf_sample_guided(B, n, _lib.ptr(t["z"]), _lib.ptr(t["depth"]), _lib.ptr(t["w"]), _lib.ptr(t["nf"]),
                                               _lib.ptr(valid), _lib.ptr(t["tdep"] if train else None), d["tdep"].shape[1],
                                               _lib.ptr(t["tstd"] if train else None), _lib.ptr(t["u_pred"]),
                                               _lib.ptr(t["u_gt"] if train else None), _lib.ptr(zs), _lib.ptr(zu), None,
                                               _lib.stream_of(zs)), "sample_guided")
    return rows_of(zs, B), rows_of(zu, B)


def check_guided_exact(d, zs, zu):
    n = d["z"].shape[1]
    assert np.isfinite(zu).all()
    assert zu[:, :n].tobytes() == d["z"].tobytes(), "z_unsort[:, :n] is not z"
    assert (np.diff(zu[:, n:], axis=-1) >= 0).all(), "z_unsort[:, n:] is not ascending"
    assert zs.tobytes() == np.sort(zu, -1).tobytes(), "z_sorted is not sort(z_unsort)"


@pytest.mark.parametrize("N", sorted(sc.SIGMA_CASES))
def test_sample_3sigma_matches_float64(N):
    d = sc.sigma_case(N)
    got = run_3sigma(d)
    p = sn.sample_3sigma(d["low"], d["high"], N, d["near"], d["far"], d["u"])
    sc.check_cap(p, f"sample_3sigma N={N}")
    sc.check_values(got, p, 2 * sc.K_ORACLE["sigma", N], f"sample_3sigma N={N}")
    out = (d["high"] < d["near"]) | (d["low"] > d["far"])       # wholly outside: every sample IS the bound
    bound = np.where(d["high"] < d["near"], d["near"], d["far"]).astype(np.float32)
    assert (got[out] == bound[out, None]).all()
    assert N < 64 or out.sum() >= 2


@pytest.mark.parametrize("nb,nd", sorted(sc.PDF_CASES))
def test_sample_pdf_matches_float64(nb, nd):
    d = sc.pdf_case(nb, nd)
    B = d["w"].shape[0]
    out = out_rows(B, nd)
    bins, w, u = dev(d["bins"]), dev(d["w"]), dev(d["u"])
    _lib.check(_lib.lib().spnerf_sample_pdf(B, nb, _lib.ptr(bins), _lib.ptr(w), nd, _lib.ptr(u), 1e-5, _lib.ptr(out), None,
                                            _lib.stream_of(out)), "sample_pdf")
    p = sn.sample_pdf(d["bins"], d["w"], d["u"])
    sc.check_cap(p, f"sample_pdf {nb} bins")
    sc.check_values(rows_of(out, B), p, 2 * sc.K_ORACLE["pdf", nb, nd], f"sample_pdf {nb} bins, {nd} draws")


@pytest.mark.parametrize("nb", [64, 128])
def test_draw_on_a_cdf_entry_starts_its_bin(nb):
    """searchsorted(right = True): u == c_k selects bin k, and the sample is b_k bit for bit"""
    d = sc.entry_case(nb)
    out = out_rows(5, nb)
    bins, w, u = dev(d["bins"]), dev(d["w"]), dev(d["u"])
    _lib.check(_lib.lib().spnerf_sample_pdf(5, nb, _lib.ptr(bins), _lib.ptr(w), nb, _lib.ptr(u), 1e-5, _lib.ptr(out), None,
                                            _lib.stream_of(out)), "sample_pdf")
    got = rows_of(out, 5)
    assert got.tobytes() == d["bins"][:, :nb].tobytes(), f"{int((got != d['bins'][:, :nb]).sum())} samples are not their bin's edge"


@pytest.mark.parametrize("mode", ["train", "test"])
@pytest.mark.parametrize("n", sorted(sc.GUIDED_CASES))
def test_guided_matches_float64(n, mode):
    d = sc.guided_case(n, mode == "train")
    zs, zu = run_guided(d)
    check_guided_exact(d, zs, zu)
    p = sc.guided_ref(d)[2]
    sc.check_cap(p, f"guided {mode} n={n}")
    K = 2 * sc.K_ORACLE["guided", n, mode]
    sc.check_sorted(zu[:, n:], p, K, f"guided {mode} n={n} z_unsort[:, n:]")
    sc.check_sorted(zs, p, K, f"guided {mode} n={n} z_sorted", exact=d["z"].astype(np.float64))


@pytest.mark.parametrize("S", sorted(sc.STRAT_CASES))
def test_stratified_matches_float64(S):
    d = sc.strat_case(S)
    B, stride = d["rays"].shape
    rays, u, z = dev(d["rays"]), dev(d["u"]), out_rows(B, S)
    _lib.check(_lib.lib().spnerf_sample_stratified(B, S, _lib.ptr(rays), stride, _lib.ptr(u), _lib.ptr(z), None,
                                                   _lib.stream_of(z)), "sample_stratified")
    got = rows_of(z, B)
    want = sn.stratified(d["rays"], S, d["u"])
    bound = 4 * sc.ULP * np.abs(d["rays"][:, 6:8]).max(-1, keepdims=True)   # the four roundings of the expression
    err = np.abs(got - want)
    print(f"stratified S={S}: worst error / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()


# ---- degenerate windows: n finite copies of the clamped centre (spnerf_amd.h) -----------------

def test_zero_width_windows_give_the_clamped_centre():
    for N in sc.ZERO_WIDTH_N:
        d = sc.zero_width_case(N)
        got = run_3sigma(d)
        want = np.clip(d["low"], sc.NEAR, sc.FAR)
        assert (got == want[:, None]).all(), N


@pytest.mark.parametrize("n", sc.DEGENERATE_N)
def test_guided_on_degenerate_rays(n):
    """sampling_cases.degenerate_guided_case: five zero-width windows next to ordinary rays"""
    d = sc.degenerate_guided_case(n)
    zs, zu = run_guided(d)
    check_guided_exact(d, zs, zu)
    centre = np.clip(d["centre"], sc.NEAR, sc.FAR)
    assert (zu[list(sc.DEGENERATE_ROWS), n:] == centre[:, None]).all()
    p = sc.guided_ref(d)[2]
    K = 2 * sc.K_ORACLE["guided_deg", n]
    sc.check_sorted(zu[:, n:], p, K, f"degenerate guided n={n} z_unsort[:, n:]")
    sc.check_sorted(zs, p, K, f"degenerate guided n={n} z_sorted", exact=d["z"].astype(np.float64))


def test_fixture_degenerate_rows():
    """the rows on which unit_sampling_shapes.npz records NaN from the reference"""
    import golden_util as gu
    with np.load(f"{gu.GOLDEN}/unit_sampling_shapes.npz") as z:
        fx = {k: z[k] for k in z.files}
    assert np.isnan(fx["deg_out"]).all()
    got = run_3sigma(dict(low=fx["deg_low"], high=fx["deg_high"], near=fx["near"], far=fx["far"], u=fx["deg_u"]))
    assert (got == np.clip(fx["deg_low"], fx["near"], fx["far"])[:, None]).all()
    d = {k: fx["degg_" + k] for k in ("z", "depth", "w", "valid", "tdep", "tstd", "u_pred")}
    d["nf"] = np.array([fx["near"], fx["far"]], np.float32)
    d["u_gt"] = np.zeros_like(d["u_pred"])
    d["u_gt"][d["valid"] > 0] = fx["degg_u_gt"]
    zs, zu = run_guided(d)
    check_guided_exact(d, zs, zu)
    nan_rows = np.isnan(fx["degg_z2"]).all(-1)
    assert nan_rows.tolist() == [True, True, True, False, True, False, False, False]
    centre = np.clip(np.where(d["valid"] > 0, d["tdep"][:, 0], d["depth"]), fx["near"], fx["far"])
    assert (zu[nan_rows, 8:] == centre[nan_rows, None]).all()
