"""The validation loss — CPU only.  The fp64 restatement (tests/val_loss_numpy.py) against what the
reference's render_rays + SNerfLoss / SatNerfLoss computed (tests/golden/val_loss.npz, made by
gen_val_golden.py): the restatement is pinned here before the kernels are held to it.

The reference sums in float32.  A float32 sum of n same-signed terms, each a rounded product, is
within (n + 1) · 2^-24 of the exact one relative to the sum of the magnitudes, in any order; a term
of the loss is a sum over the S' samples of a ray and then a mean over the N rays (or over 3N colour
values), so (S' + 3N + 8) · 2^-24 bounds it, the 8 covering the divisions, the λ / 3 factor and the
float32 targets.  term3 = 1 − Σ w·sun and logbeta = (3 + mean log b) / 2 are differences: their
bound is relative to the magnitudes that enter (λ / 3 · 1 and 3 / 2 + |mean log b| / 2)."""
import numpy as np
import pytest

import val_loss_numpy as vl

EPS = 2.0 ** -24


def term_bounds(d, ref_terms):
    a = d["meta"]["args"]
    n = d["meta"]["n_rays"]
    S = d["out_z_vals_coarse"].shape[1] + a["n_importance"]
    rel = (S + 3 * n + 8) * EPS
    lam = a["sc_lambda"]
    out = {}
    for k, v in ref_terms.items():
        mag = abs(v)
        if k.endswith("sc_term3"):
            mag = lam / 3.0 * 2.0 - v          # λ/3 · (1 + mean Σ w·sun)
        if k.endswith("logbeta"):
            mag = 1.5 + abs(v - 1.5)
        out[k] = rel * mag
    return out


@pytest.mark.parametrize("case", vl.CASES)
def test_restatement_matches_reference(case):
    d = vl.load_case(case)
    a = d["meta"]["args"]
    assert d["rays"].shape == (37, 11) and d["target"].shape == (37, 3)
    p = vl.reference_planes(d)
    got = vl.view_loss(p["rgb"], p["target"], a["sc_lambda"], p.get("term2"), p.get("term3"), p.get("beta"),
                       rgb_coarse=p.get("rgb_coarse"))
    ref = d["terms"]
    assert sorted(got) == sorted(list(ref) + ["loss"])
    expected = {"a": ["coarse_color", "coarse_sc_term2", "coarse_sc_term3"], "d": ["coarse_color", "coarse_logbeta",
                "coarse_sc_term2", "coarse_sc_term3"], "e": ["coarse_color", "fine_color"]}
    assert sorted(ref) == expected.get(case, expected["a"])
    tol = term_bounds(d, ref)
    for k, v in ref.items():
        print(case, k, got[k], v, f"err {abs(got[k] - v):.2e} bound {tol[k]:.2e}")
        assert abs(got[k] - v) <= tol[k], (case, k, got[k], v)
    assert abs(got["loss"] - d["loss"]) <= sum(tol.values()) + EPS * abs(d["loss"])


def test_fixture_covers_the_lane_layouts():
    """S' of the solar cases: below the 64 lanes, two samples per lane with a ragged tail, and the
    draws in the validation step's order — the solar pass's noise right after the main pass's."""
    S = {c: vl.load_case(c)["out_z_vals_coarse"].shape[1] for c in vl.CASES}
    assert S == {"a": 48, "b": 40, "c": 96, "d": 32, "e": 32}
    for c in vl.SOLAR_CASES:
        d = vl.load_case(c)
        draws = sorted(k for k in d if k.startswith("rng"))
        assert draws[-1].endswith("randn") and draws[-2].endswith("randn")
        assert d[draws[-1]].shape == d[draws[-2]].shape == (37, S[c])
        assert d["out_sun_sc_coarse"].shape == (37, S[c], 1) and d["out_weights_sc_coarse"].shape == (37, S[c])
    e = vl.load_case("e")
    assert e["out_rgb_fine"].shape == (37, 3) and e["out_z_vals_fine"].shape == (37, 48) and "out_sun_sc_coarse" not in e
    assert vl.load_case("b")["meta"]["args"]["noise_std"] == 0.3


def test_march_matches_the_reference_solar_pass():
    """``march`` on the solar pass's own densities is not stored; its laws are: an empty ray keeps
    T = 1 up to the 1e-10 factors and w = 0, an opaque first sample takes all the weight."""
    z = np.linspace(0.0, 0.2, 7)[None].repeat(2, 0)
    sig = np.zeros((2, 7))
    sig[1, 0] = 1e4
    T, w = vl.march(sig, z)
    assert np.allclose(T[0], 1.0, atol=1e-8) and np.all(w[0] == 0.0)
    assert T[1, 0] == 1.0 and abs(w[1, 0] - 1.0) < 1e-12 and np.all(T[1, 1:] < 2e-10 + np.exp(-1e4 * 0.2 / 6))
    sun = np.full((2, 7), 0.25)
    t2, t3 = vl.solar_terms(T, w, sun)
    assert abs(t3[0] - 1.0) < 1e-12 and abs(t2[0] - 7 * 0.75 ** 2) < 1e-7
    assert abs(t3[1] - 0.75) < 1e-9 and abs(t2[1] - (0.75 ** 2 + 6 * 0.25 ** 2)) < 1e-7
    # a single sample: δ = 1e10, T = 1
    T1, w1 = vl.march(np.array([[0.5]]), np.array([[0.1]]))
    assert T1[0, 0] == 1.0 and w1[0, 0] == 1.0


def test_view_loss_sums_the_terms_present():
    g = np.random.default_rng(0)
    rgb, tgt = g.uniform(size=(5, 3)), g.uniform(size=(5, 3))
    plain = vl.view_loss(rgb, tgt)
    assert sorted(plain) == ["coarse_color", "loss"] and plain["loss"] == plain["coarse_color"]
    t2, t3 = g.uniform(size=5), g.uniform(size=5)
    sc = vl.view_loss(rgb, tgt, 0.3, t2, t3)
    assert abs(sc["coarse_sc_term2"] - 0.1 * t2.mean()) < 1e-15 and abs(sc["coarse_sc_term3"] - 0.1 * t3.mean()) < 1e-15
    assert abs(sc["loss"] - (plain["loss"] + 0.1 * (t2.mean() + t3.mean()))) < 1e-15
    b = g.uniform(0.01, 0.5, 5)
    sat = vl.view_loss(rgb, tgt, beta=b)
    assert abs(sat["coarse_color"] - np.mean((rgb - tgt) ** 2 / (2 * (b[:, None] + 0.05) ** 2))) < 1e-15
    assert abs(sat["coarse_logbeta"] - (3 + np.log(b + 0.05).mean()) / 2) < 1e-15
    fine = vl.view_loss(rgb, tgt, rgb_coarse=tgt)
    assert fine["coarse_color"] == 0.0 and fine["fine_color"] == plain["coarse_color"]
