"""fp64 numpy restatement of the validation loss (the reference's modules/metrics.py:
uncertainty_aware_loss :10, solar_correction :17, SNerfLoss :27, SatNerfLoss :48) in the per-ray
form the library computes it in, and the loader of its fixture (tests/golden/val_loss.npz, made by
tests/golden/gen_val_golden.py).

``solar_terms`` are the two per-ray sums of the solar pass; ``march`` is the per-sample α / T / w of
a ray (models/spnerf.py:115-128) for rows that have no reference run; ``view_loss`` forms the terms
and their sum from per-ray planes, everything in float64."""
from __future__ import annotations

import ast
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "val_loss.npz")
CASES = ("a", "b", "c", "d", "e")
SOLAR_CASES = ("a", "b", "c", "d")


def march(sigma, z, noise=None, noise_std=0.0):
    """(T, w) of rays with densities ``sigma`` (B, S) at depths ``z`` (B, S): α = 1 − exp(−δ·relu(σ + noise·std)),
    δ the depth steps with 1e10 for the last, T the exclusive product of 1 − α + 1e-10, w = α·T."""
    sigma, z = np.asarray(sigma, np.float64), np.asarray(z, np.float64)
    if noise is not None:
        sigma = sigma + np.asarray(noise, np.float64) * noise_std
    delta = np.concatenate([z[:, 1:] - z[:, :-1], np.full_like(z[:, :1], 1e10)], -1)
    alpha = 1.0 - np.exp(-delta * np.maximum(sigma, 0.0))
    t = 1.0 - alpha + 1e-10
    T = np.concatenate([np.ones_like(t[:, :1]), np.cumprod(t, -1)[:, :-1]], -1)
    return T, alpha * T


def solar_terms(transparency, weights, sun):
    """(term2, term3) per ray: Σ_s (T_s − sun_s)² and 1 − Σ_s w_s·sun_s (metrics.py:20-21)."""
    T, w = np.asarray(transparency, np.float64), np.asarray(weights, np.float64)
    sun = np.asarray(sun, np.float64).reshape(T.shape)
    return np.sum((T - sun) ** 2, -1), 1.0 - np.sum(w * sun, -1)


def view_loss(rgb, target, lambda_sc=0.0, term2=None, term3=None, beta=None, beta_min=0.05, rgb_coarse=None) -> dict:
    """``loss`` and the reference's ``loss_dict`` from per-ray planes.  ``rgb`` is the fine colour
    when ``rgb_coarse`` is given; ``beta`` is Σ w·β per ray (SatNerfLoss), None for SNerfLoss; the
    solar terms enter when ``lambda_sc > 0``."""
    rgb, target = np.asarray(rgb, np.float64).reshape(-1, 3), np.asarray(target, np.float64).reshape(-1, 3)
    sq = (rgb - target) ** 2
    out = {}
    if beta is not None:
        b = np.asarray(beta, np.float64).reshape(-1, 1) + beta_min
        out["coarse_color"] = float(np.mean(sq / (2.0 * b ** 2)))
        out["coarse_logbeta"] = float((3.0 + np.mean(np.log(b))) / 2.0)
    elif rgb_coarse is not None:
        out["coarse_color"] = float(np.mean((np.asarray(rgb_coarse, np.float64).reshape(-1, 3) - target) ** 2))
        out["fine_color"] = float(np.mean(sq))
    else:
        out["coarse_color"] = float(np.mean(sq))
    if lambda_sc > 0:
        out["coarse_sc_term2"] = float(lambda_sc / 3.0 * np.mean(np.asarray(term2, np.float64)))
        out["coarse_sc_term3"] = float(lambda_sc / 3.0 * np.mean(np.asarray(term3, np.float64)))
    out["loss"] = float(sum(out.values()))
    return out


def load_case(case: str) -> dict:
    """One case of the fixture in golden_util.load's form: its arrays without the ``<case>|``
    prefix, ``meta`` as a dictionary and ``terms``: the reference's loss_dict."""
    with np.load(GOLDEN, allow_pickle=False) as z:
        data = {k.split("|", 1)[1]: z[k] for k in z.files if k.startswith(case + "|")}
    data["meta"] = ast.literal_eval(str(data.pop("meta")))
    data["terms"] = {k.split("|", 1)[1]: float(data.pop(k)) for k in sorted(data) if k.startswith("term|")}
    data["loss"] = float(data["loss"])
    return data


def reference_planes(d: dict) -> dict:
    """What the restatement reads of a fixture case: the reference's per-sample tensors reduced to
    per-ray planes in float64."""
    p = {"target": d["target"]}
    fine = "out_rgb_fine" in d
    p["rgb"] = d["out_rgb_fine"] if fine else d["out_rgb_coarse"]
    if fine:
        p["rgb_coarse"] = d["out_rgb_coarse"]
    if "out_sun_sc_coarse" in d:
        p["term2"], p["term3"] = solar_terms(d["out_transparency_sc_coarse"], d["out_weights_sc_coarse"], d["out_sun_sc_coarse"])
    if "out_beta_coarse" in d:
        p["beta"] = np.sum(d["out_weights_coarse"].astype(np.float64)[..., None] * d["out_beta_coarse"].astype(np.float64), -2)[:, 0]
    return p
