"""The numpy statement of the confidence planes (tests/confidence_numpy.py) pinned to closed forms, the frozen cases
(tests/confidence_cases.py) to what they claim to be, and ``sparsification`` to its statement — no GPU needed."""
import math

import numpy as np
import torch

import abi_util
import confidence_cases as cc
import confidence_numpy as cn
from spnerf_amd import _confidence_abi, confidence

F = np.float32
HEADER = abi_util.header_path("staged/spnerf_amd_confidence.h")


def column(values):
    return np.asarray(values, F)[:, None]


def one(values, step=0.5, tau=0.05, temperature=0.1, exclude=1):
    return {k: v[0] for k, v in cn.confidence(column(values), step, tau, temperature, exclude).items()}


def test_the_headers_constants_are_the_tables():
    consts = abi_util.defines(HEADER, "SPNERF_CONF_")
    assert consts["SPNERF_CONF_ABI_VERSION"] == _confidence_abi.SPNERF_CONF_ABI_VERSION == 1
    assert consts["SPNERF_CONF_MAX_PLANES"] == _confidence_abi.CONF_MAX_PLANES == confidence.MAX_PLANES == 512 == max(cc.PLANE_COUNTS)
    assert consts["SPNERF_CONF_OUTPUTS"] == len(_confidence_abi.CONF_OUTPUTS) == len(cn.PLANES) == 9
    assert confidence.PLANES == cn.PLANES == tuple(n for n, _ in _confidence_abi.CONF_OUTPUTS)
    text = open(HEADER).read()
    order = [text.index(f"\n *   {name} ") for name in cn.PLANES]           # the definition names the planes in the pointers' order
    assert order == sorted(order)
    assert (confidence.TAU, confidence.TEMPERATURE) == (0.1, 0.2)          # the rows chosen on the ROI


def test_a_lone_scored_plane():
    for K in cc.PLANE_COUNTS:
        got = one(cc.one_scored(K))
        assert (got["scored"], got["index"], got["peaks"], got["support"]) == (1, K // 2, 1, 1)
        assert got["mlm"] == 1 and got["spread"] == 0
        assert np.isnan(got["margin"]) and np.isnan(got["peak_margin"]) and np.isnan(got["curvature"])
    got = one(cc.all_nan(5))
    assert (got["scored"], got["index"], got["peaks"], got["support"]) == (0, -1, 0, 0)
    assert all(np.isnan(got[k]) for k in ("margin", "peak_margin", "curvature", "mlm", "spread"))


def test_two_equal_peaks():
    K, T, low, top = 64, 0.1, 0.25, 0.7
    col = cc.equal_peaks(K)
    assert col[16] == col[47] == F(top) and (np.delete(col, [16, 47]) == F(low)).all() and 47 - 16 == 31
    d = 31
    got = one(col, step=0.5, tau=0.05, temperature=T)
    assert (got["index"], got["margin"], got["peak_margin"], got["peaks"], got["support"]) == (16, 0, 0, 2, 2)
    # the other planes' stated weights: w each, K − 2 of them, at their distances from the pick
    w = math.exp((float(F(low)) - float(F(top))) / float(F(T)))
    Z = 2 + (K - 2) * w
    assert abs(got["mlm64"] - 1 / Z) < 1e-15 and abs(1 / Z - 0.5) < 0.2
    second = sum(w * (k - 16) ** 2 for k in range(K) if k not in (16, 47))
    assert abs(got["spread64"] - 0.5 * math.sqrt((d * d + second) / Z)) < 1e-12
    # alone in the column: exactly 1/2 and step·d/√2
    bare = np.full(K, np.nan, F)
    bare[[16, 47]] = top
    got = one(bare)
    assert got["mlm64"] == 0.5 and abs(got["spread64"] - 0.5 * d / math.sqrt(2)) < 1e-14 and got["scored"] == 2
    # inside exclude the second peak is the pick's own: no margin, but a peak_margin
    got = one(cc.second_peak(64, 1), exclude=1)
    assert got["margin"] == F(0.9) - F(0.25) and got["peak_margin"] == F(0.9) - F(0.25) and got["peaks"] == 1
    got = one(cc.second_peak(64, 2), exclude=1, tau=0.04)
    assert got["margin"] == got["peak_margin"] == F(0.9) - F(0.85) and got["peaks"] == 1
    assert one(cc.second_peak(64, 2), exclude=2)["margin"] == F(0.9) - F(0.25)
    assert one(cc.second_peak(64, 2), tau=0.06)["peaks"] == 2
    assert np.isnan(one(cc.second_peak(64, 2), exclude=64)["margin"])


def test_a_flat_row_a_plateau_and_ties():
    for K in cc.PLANE_COUNTS:
        got = one(cc.flat(K), tau=0.0)
        assert (got["index"], got["scored"], got["support"], got["peaks"]) == (0, K, K, 1)
        assert abs(got["mlm64"] - 1 / K) < 1e-15
        assert np.isnan(got["peak_margin"]) and (np.isnan(got["margin"]) if K <= 2 else got["margin"] == 0)
    got = one(cc.plateau(64))
    assert (got["index"], got["peaks"], got["support"], got["margin"]) == (21, 1, 3, 0)       # counted once, at its lowest plane
    assert got["peak_margin"] == F(0.8) - F(0.25) and got["curvature"] == F(0.8) - F(0.25)     # the other maximum is the floor's plateau at plane 0
    got = one(cc.tie_with_neighbour(64), tau=0.0)
    assert (got["index"], got["peaks"], got["support"]) == (62, 1, 2) and np.isnan(got["peak_margin"])


def test_a_parabolas_curvature_is_its_second_difference():
    k = np.arange(9, dtype=np.float64)
    col = (0.875 - 0.0078125 * (k - 4) ** 2).astype(F)                      # exact in fp32
    got = one(col)
    assert got["index"] == 4 and got["curvature"] == F(2 * 0.0078125)
    assert np.isnan(one(cc.pick_at_bottom(9))["curvature"]) and np.isnan(one(cc.pick_at_top(9))["curvature"])
    assert np.isnan(one(cc.unscored_neighbour(9))["curvature"]) and one(cc.unscored_neighbour(9))["index"] == 4


def test_infinities_are_unscored_and_tau_is_met_exactly():
    got = one(cc.infinities(9))
    assert (got["scored"], got["index"]) == (7, 7) and np.isnan(got["curvature"])
    for ulps, want in ((0, 2), (1, 1)):
        col = cc.tau_cell(64, ulps)
        assert np.float64(col[0]) - np.float64(col[63]) == cc.TAU_EXACT + ulps * 2.0 ** -24
        got = one(col, tau=cc.TAU_EXACT)
        assert (got["index"], got["peaks"], got["support"]) == (0, want, want)
    assert one(cc.tau_cell(64, 0), tau=0.0)["peaks"] == 1


def test_the_random_columns_carry_weight_at_every_plane():
    v = cc.random_columns(64, 257, 1)
    share = np.isnan(v).mean()
    assert 0.27 < share < 0.33
    best = np.nanmax(v, axis=0)
    assert (best - np.nanmin(v, axis=0) <= 4 * cc.TEMPERATURE + 1e-6).all()
    assert cc.volume(512, 257).shape == (512, 257) and cc.volume(1, 1).shape == (1, 1)


def test_sparsification_against_its_statement_and_closed_forms():
    rng = np.random.default_rng(5)
    err = rng.uniform(0, 3, (20, 31))
    conf = np.round(rng.uniform(0, 1, err.shape), 1)                      # many ties: the cell index decides
    err[3, 4], conf[7, 8], conf[9, 9] = np.nan, np.nan, np.inf
    for steps in (100, 7):
        got = confidence.sparsification(torch.tensor(err), torch.tensor(conf, dtype=torch.float32), steps=steps)
        curve, area = cn.sparsification(err, conf.astype(F), steps)
        assert got["cells"] == err.size - 3 and got["curve"].dtype == torch.float64
        assert np.allclose(got["curve"].numpy(), curve, rtol=1e-12, atol=0) and abs(got["area"] - area) < 1e-12
    # the oracle: confidence = −error removes the largest errors first; error 1..n has a closed form
    n, steps = 1000, 100
    ramp = torch.arange(1, n + 1, dtype=torch.float64)
    oracle = confidence.sparsification(ramp, -ramp, steps=steps)
    want = np.array([(n - n * i // steps + 1) / 2 for i in range(steps)])
    assert np.allclose(oracle["curve"].numpy(), want, rtol=1e-13)
    assert abs(oracle["area"] - sum((want[i] + want[i + 1]) / 2 / steps for i in range(steps - 1)) / want[0]) < 1e-13
    shuffled = torch.tensor(rng.permutation(n) + 1.0)
    assert abs(confidence.sparsification(shuffled, -shuffled, steps=steps)["area"] - oracle["area"]) < 1e-13
    worst = confidence.sparsification(shuffled, shuffled, steps=steps)
    assert worst["area"] > 1 > oracle["area"] and (np.diff(oracle["curve"].numpy()) < 0).all()
    # a constant confidence keeps the cells of the lowest index: over a constant or a period-2 error that is flat
    for e in (torch.full((n,), 2.5, dtype=torch.float64), torch.tensor([1.0, 3.0] * (n // 2), dtype=torch.float64)):
        flat = confidence.sparsification(e, torch.zeros(n), steps=steps)
        assert (flat["curve"] == flat["curve"][0]).all() and abs(flat["area"] - (1 - 1 / steps)) < 1e-13


def test_sparsification_refuses_bad_arguments():
    import pytest
    e = torch.zeros(4, 5)
    for args, kw, text in (((e.numpy(), e), {}, "error must be a non-empty floating-point tensor"), ((e, e.int()), {}, "confidence must be"),
                           ((e, e[:3]), {}, "confidence \\(3, 5\\) is not error's \\(4, 5\\)"), ((e, e), dict(steps=1), "steps 1 must be an integer in 2"),
                           ((e, e.to("meta")), {}, "on one device")):
        with pytest.raises(ValueError, match=text):
            confidence.sparsification(*args, **kw)
    empty = confidence.sparsification(e * float("nan"), e, steps=5)
    assert empty["cells"] == 0 and math.isnan(empty["area"]) and empty["curve"].shape == (5,)
