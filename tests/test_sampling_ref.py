"""The float64 restatement of the depth samplers (tests/sampling_numpy.py) against the reference's
own results, and the inputs of tests/test_gpu_sampling.py vetted on the CPU.

  * the restatement equals what the reference returned (tests/golden/unit_sampling_shapes.npz,
    written by gen_sampling_golden.py, and the older unit_sampling.npz) within the value bound of
    tests/sampling_cases.py at the K of the nearest listed shape, doubled — the reference is float32
    torch, exactly what K_ORACLE was measured on;
  * on the degenerate rows the fixture records NaN from the reference; the restatement states the
    library's contract there (n copies of the clamped window centre);
  * oracle/ref_cpu.py against the restatement on every input of the GPU module: the K it needs is
    printed and must not exceed 1.1 times its K_ORACLE entry, so the table stays what the oracle
    measures (the tenth is for hosts whose vector width makes torch sum a row in another order);
  * the ambiguity mask's leave-out cap on every one of those inputs, from the restatement alone: a
    badly chosen input fails here and not silently on the GPU.
"""
import numpy as np
import pytest
import torch

import golden_util as gu
import sampling_cases as sc
import sampling_numpy as sn
from oracle import ref_cpu

T = torch.tensor


@pytest.fixture(scope="module")
def fx():
    with np.load(f"{gu.GOLDEN}/unit_sampling_shapes.npz") as z:
        return {k: z[k] for k in z.files}


# ---- the restatement against the reference's recorded results --------------------------------

@pytest.mark.parametrize("N", sorted(sc.SIGMA_CASES))
def test_sample_3sigma_matches_reference(fx, N):
    g = lambda k: fx[f"s3_{N}_{k}"]
    p = sn.sample_3sigma(g("low"), g("high"), N, fx["near"], fx["far"], g("u"))
    sc.check_cap(p, f"fixture sample_3sigma N={N}")
    sc.check_values(g("out"), p, 2 * sc.K_ORACLE["sigma", N], f"reference sample_3sigma N={N}")


@pytest.mark.parametrize("nb,nd", sorted(sc.PDF_CASES))
def test_sample_pdf_matches_reference(fx, nb, nd):
    g = lambda k: fx[f"pdf_{nb}_{nd}_{k}"]
    p = sn.sample_pdf(g("bins"), g("w"), g("u"))
    assert p.s.shape == (10, nd)
    sc.check_cap(p, f"fixture sample_pdf {nb} bins")
    sc.check_values(g("out"), p, 2 * sc.K_ORACLE["pdf", nb, nd], f"reference sample_pdf {nb} bins, {nd} draws")


def fixture_guided(fx, key):
    d = {k: fx[key + k] for k in ("z", "depth", "w", "valid", "tdep", "tstd", "u_pred")}
    train = key.startswith(("g_train", "degg"))
    u_gt = np.zeros_like(d["u_pred"])
    if train:
        u_gt[d["valid"] > 0] = fx[key + "u_gt"]              # the reference draws rows for the valid rays only
    nf = np.array([fx["near"], fx["far"]], np.float32)
    return sn.guided(d["z"], d["depth"], d["w"], nf, d["valid"] if train else None, d["tdep"][:, 0], d["tstd"],
                     d["u_pred"], u_gt, detail=True), d


@pytest.mark.parametrize("mode", ["train", "test"])
@pytest.mark.parametrize("n", sorted(sc.GUIDED_CASES))
def test_guided_matches_reference(fx, n, mode):
    key = f"g_{mode}_{n}_"
    (zs, zu, p), d = fixture_guided(fx, key)
    K = 2 * sc.K_ORACLE["guided", n, mode]
    sc.check_cap(p, key)
    sc.check_values(fx[key + "z2"], p, K, f"reference GenerateGuidedSamples {mode} n={n}")
    np.testing.assert_array_equal(fx[key + "unsort"][:, :n], d["z"])
    sc.check_sorted(fx[key + "unsort"][:, n:], p, K, key + "unsort")
    sc.check_sorted(fx[key + "sorted"], p, K, key + "sorted", exact=d["z"].astype(np.float64))


def test_existing_unit_fixture():
    """unit_sampling.npz (N = 64 windows; 32 bins, 40 draws) at the K of the 64-edge shapes"""
    with np.load(f"{gu.GOLDEN}/unit_sampling.npz") as z:
        d = {k: z[k] for k in z.files}
    p = sn.sample_3sigma(d["low"], d["high"], 64, np.float32(d["near"]), np.float32(d["far"]), d["u3"])
    sc.check_values(d["s3"], p, 2 * sc.K_ORACLE["sigma", 64], "unit_sampling sample_3sigma")
    p = sn.sample_pdf(d["bins"], d["w"], d["u_pdf"])
    sc.check_values(d["s_pdf"], p, 2 * sc.K_ORACLE["pdf", 64, 64], "unit_sampling sample_pdf")


def test_reference_returns_nan_on_zero_width_windows(fx):
    """recorded, not endorsed: the library returns the clamped centre there (spnerf_amd.h)"""
    assert np.isnan(fx["deg_out"]).all()
    p = sn.sample_3sigma(fx["deg_low"], fx["deg_high"], 8, fx["near"], fx["far"], fx["deg_u"])
    centre = np.clip(fx["deg_low"], fx["near"], fx["far"]).astype(np.float64)
    np.testing.assert_array_equal(p.s, np.repeat(centre[:, None], 8, 1))
    (zs, zu, p), d = fixture_guided(fx, "degg_")
    bad = np.array([0, 1, 2, 4])          # one-sample weight, empty ray, GT spread 0, one-sample weight at z[0]
    ok = np.array([3, 5, 6, 7])
    assert np.isnan(fx["degg_z2"][bad]).all() and np.isfinite(fx["degg_z2"][ok]).all()
    want = np.clip(np.array([d["depth"][0], 0.0, d["tdep"][2, 0], d["depth"][4]], np.float32), fx["near"], fx["far"])
    np.testing.assert_array_equal(p.s[bad], np.repeat(want.astype(np.float64)[:, None], 8, 1))
    sc.check_sorted(fx["degg_sorted"][ok], sc.rows(p, ok), 2 * sc.K_ORACLE["guided", 5, "test"], "degg_sorted",
                    exact=d["z"][ok].astype(np.float64))


def test_stratified_matches_oracle():
    for S in sc.STRAT_CASES:
        d = sc.strat_case(S)
        want = sn.stratified(d["rays"], S, d["u"])
        got = ref_cpu.stratified(T(d["rays"]), S, T(d["u"])).numpy()
        bound = 4 * sc.ULP * np.abs(d["rays"][:, 6:8]).max(-1, keepdims=True)
        assert (np.abs(got - want) <= bound).all(), S


# ---- the GPU module's inputs: the oracle's K and the leave-out cap ---------------------------

def _oracle(what, got, p, key):
    sc.check_cap(p, what)
    need, worst = sc.k_needed(got, p)
    print(f"{what}: oracle K {need:.3g} (listed {sc.K_ORACLE[key]}), worst kept error {worst:.3e}, "
          f"left out {p.amb.mean():.2%}")
    assert need <= 1.1 * sc.K_ORACLE[key], f"{what}: the oracle needs K {need:.4g}, the table lists {sc.K_ORACLE[key]}"
    sc.check_values(got, p, 1.1 * sc.K_ORACLE[key], what)


@pytest.mark.parametrize("N", sorted(sc.SIGMA_CASES))
def test_gpu_inputs_sample_3sigma(N):
    d = sc.sigma_case(N)
    assert d["u"][:, 0].max() == 0.0 and d["u"][:, -1].min() == np.float32(1 - sc.ULP)
    got = ref_cpu.sample_3sigma(T(d["low"]), T(d["high"]), N, T(d["near"]), T(d["far"]), T(d["u"])).numpy()
    _oracle(f"sample_3sigma N={N}", got, sn.sample_3sigma(d["low"], d["high"], N, d["near"], d["far"], d["u"]), ("sigma", N))


@pytest.mark.parametrize("nb,nd", sorted(sc.PDF_CASES))
def test_gpu_inputs_sample_pdf(nb, nd):
    d = sc.pdf_case(nb, nd)
    got = ref_cpu.sample_pdf(T(d["bins"]), T(d["w"]), T(d["u"])).numpy()
    _oracle(f"sample_pdf {nb} bins, {nd} draws", got, sn.sample_pdf(d["bins"], d["w"], d["u"]), ("pdf", nb, nd))


@pytest.mark.parametrize("mode", ["train", "test"])
@pytest.mark.parametrize("n", sorted(sc.GUIDED_CASES))
def test_gpu_inputs_guided(n, mode):
    d = sc.guided_case(n, mode == "train")
    zs, zu, p = sc.guided_ref(d)
    _oracle(f"guided {mode} n={n}", sc.oracle_guided(d), p, ("guided", n, mode))
    if mode == "train" and n >= 64:
        # the two windows of a valid ray lie far apart next to the bound: the wrong window, or the
        # other row of draws, misses by a wide margin
        other = dict(d, u_gt=d["u_pred"])
        moved = np.abs(sc.guided_ref(other)[2].s - p.s)[d["valid"] > 0]
        assert (moved.max(-1) > 1e3 * sc.tol_of(p, 2 * sc.K_ORACLE["guided", n, mode])[d["valid"] > 0].max(-1)).mean() > 0.5
        sel = d["valid"] > 0
        gap = np.abs(d["tdep"][:, 0] - d["depth"])[sel]
        assert (gap > 0.03).all(), gap.min()


@pytest.mark.parametrize("nb", [64, 128])
def test_gpu_inputs_draw_on_a_cdf_entry(nb):
    """the oracle and the restatement return b_k bit for bit; taking the bin before it would not"""
    d = sc.entry_case(nb)
    got = ref_cpu.sample_pdf(T(d["bins"]), T(d["w"]), T(d["u"])).numpy()
    assert got.tobytes() == d["bins"][:, :nb].tobytes()
    p = sn.sample_pdf(d["bins"], d["w"], d["u"])
    np.testing.assert_array_equal(p.s, d["bins"][:, :nb].astype(np.float64))
    assert not p.amb.any()
    b = d["bins"]
    other = b[:, :-1] + np.float32(1.0) * (b[:, 1:] - b[:, :-1])
    assert (other != b[:, 1:])[:, :nb - 1].mean() > 0.1


@pytest.mark.parametrize("n", sc.DEGENERATE_N)
def test_gpu_inputs_degenerate_guided(n):
    """the oracle returns NaN on the zero-width rows and meets the listed K on the ordinary ones"""
    d = sc.degenerate_guided_case(n)
    p = sc.guided_ref(d)[2]
    sc.check_cap(p, f"degenerate guided n={n}")
    got = sc.oracle_guided(d)
    deg = sc.degenerate_mask(d)
    assert np.isnan(got[deg]).all() and np.isfinite(got[~deg]).all()
    centre = np.clip(d["centre"], sc.NEAR, sc.FAR).astype(np.float64)
    np.testing.assert_array_equal(p.s[list(sc.DEGENERATE_ROWS)], np.repeat(centre[:, None], n, 1))
    need, _ = sc.k_needed(got[~deg], sc.rows(p, ~deg))
    print(f"degenerate guided n={n}: oracle K {need:.3g} (listed {sc.K_ORACLE['guided_deg', n]})")
    assert need <= 1.1 * sc.K_ORACLE["guided_deg", n]


def test_gpu_inputs_zero_width_windows():
    for N in sc.ZERO_WIDTH_N:
        d = sc.zero_width_case(N)
        p = sn.sample_3sigma(d["low"], d["high"], N, d["near"], d["far"], d["u"])
        assert not p.amb.any()
        np.testing.assert_array_equal(p.s, np.repeat(np.clip(d["low"], sc.NEAR, sc.FAR).astype(np.float64)[:, None], N, 1))
