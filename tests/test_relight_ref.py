"""The relighting split (tests/relight_numpy.py) against oracle/ref_cpu.py's full forward and
composite with the sun columns replaced, both in float64: the two are algebraically identical, so
they agree to 1e-12 relative.  Three directions; the semantic cases and the β case of the view
fixture.  And the check of what the GPU tests use (tests/relight_cases.py: the scale of the sun
columns and the five directions): on the oracle's own ``sun`` planes over the fixture's 120 rays,
at both widths, the directions differ pairwise by at least 20x every tolerance in use — no GPU
needed."""
import dataclasses

import numpy as np
import pytest
import torch

import golden_util as gu
import relight_numpy as rn
import view_numpy as vn
from oracle import ref_cpu
from oracle.weights import make_weights
from relight_cases import BF16_TOL, DIRS as DIRS5, FP32_RTOL, SEPARATION, min_separation, scale_sun_columns

DIRS = DIRS5[[0, 2, 4]].astype(np.float64)
N_RAYS, N_SAMPLES = 12, 16


def trunk_features(p, d, xyz, labels):
    """xyz_features and the trunk output h: ref_cpu.field up to feats_from_xyz (spnerf.py:332-338)."""
    enc = ref_cpu.posenc(xyz, d.n_freq) if d.mapping else xyz
    if d.sem:
        lab = torch.where(labels == -100, torch.full_like(labels, d.num_sem_classes), labels)
        enc = torch.cat([enc, torch.nn.functional.embedding(lab, p["semantic_embedding.weight"])], 1)
    h = enc
    for i in range(d.layers):
        if i in d.skips:
            h = torch.cat([h, enc], -1)
        h = torch.sin((30.0 if i == 0 else 1.0) * ref_cpu._lin(p, f"fc_net.{2 * i}", h))
    return ref_cpu._lin(p, "feats_from_xyz", h)


@pytest.mark.parametrize("case", vn.CASES)
def test_split_equals_the_full_forward_per_direction(case):
    data = vn.load_case(case)
    meta = data["meta"]
    d = gu.dims_of(meta)
    weights = scale_sun_columns(make_weights(d, meta["seed"]), d.width)   # or the direction barely matters
    p = {k: torch.tensor(v, dtype=torch.float64) for k, v in weights.items()}
    rays = torch.tensor(data["rays"][:N_RAYS], dtype=torch.float64)
    z = ref_cpu.stratified(rays, N_SAMPLES, torch.full((N_RAYS, N_SAMPLES), 0.5, dtype=torch.float64))
    xyz = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None]).reshape(-1, 3)
    labels = torch.tensor(data["in_semantics"][:N_RAYS]).reshape(-1).long().repeat_interleave(N_SAMPLES)
    t_emb = None
    if d.beta:
        t_emb = torch.tensor(data["in_t_embedding"], dtype=torch.float64)[torch.tensor(data["in_ts"][:N_RAYS]).reshape(-1).long()]
        t_emb = t_emb.repeat_interleave(N_SAMPLES, 0)
    assert d.sem and (case != "c" or d.beta)                 # the semantic cases; c is the β case
    # the oracle: the whole network and composite once per direction
    ref = {"rgb": [], "sun": [], "sky": []}
    for k in range(3):
        sun_d = torch.tensor(DIRS[k], dtype=torch.float64).expand(xyz.shape[0], 3)
        out = ref_cpu.field(p, d, xyz, sun_d, labels, t_emb).view(N_RAYS, N_SAMPLES, -1)
        rgb, _, w, _ = ref_cpu.composite(out, z, None, 0.0)
        ref["rgb"].append(rgb.numpy())
        ref["sun"].append(torch.sum(w * out[..., 4], -1).numpy())
        ref["sky"].append(torch.sum(w[..., None] * out[..., 5:8], -2).numpy())
    # the split: the geometry (any direction's rows hold it), then the sun-dependent rest per direction
    feat = trunk_features(p, d, xyz, labels).numpy()
    pn = {k: v.numpy() for k, v in p.items()}
    albedo, wn = out[..., :3].numpy(), w.numpy()
    sun_v = rn.sun_visibility(pn, feat, DIRS).reshape(3, N_RAYS, N_SAMPLES)
    rgb, sun, sky = rn.relight_sums(wn, albedo, sun_v, rn.sky_colour(pn, DIRS))
    for name, got in (("rgb", rgb), ("sun", sun), ("sky", sky)):
        want = np.stack(ref[name])
        err = np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300))
        print(case, name, err)
        assert got.shape == want.shape and err <= 1e-12, (case, name, err)


@pytest.mark.parametrize("width", [64, 256])
@pytest.mark.parametrize("case", vn.CASES)
def test_the_gpu_tests_directions_separate_the_oracles_sun_planes(case, width):
    """The five directions and the scale of tests/relight_cases.py on oracle/ref_cpu.py's forward and
    composite, in fp32 as the model runs, over the fixture's rays at its n_samples (mid-bin depths):
    the smallest pairwise difference of the sun planes is at least 20x the fp32 tolerance and 20x the
    bf16 sun bound, with the headroom the GPU's own draws need."""
    data = vn.load_case(case)
    meta = data["meta"]
    d = dataclasses.replace(gu.dims_of(meta), width=width)
    p = {k: torch.tensor(v) for k, v in scale_sun_columns(make_weights(d, meta["seed"]), width).items()}
    rays = torch.tensor(data["rays"])
    N, S = rays.shape[0], meta["args"]["n_samples"]
    z = ref_cpu.stratified(rays, S, torch.full((N, S), 0.5))
    xyz = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None]).reshape(-1, 3)
    labels = torch.tensor(data["in_semantics"]).reshape(-1).long().repeat_interleave(S)
    t_emb = None
    if d.beta:
        t_emb = torch.tensor(data["in_t_embedding"])[torch.tensor(data["in_ts"]).reshape(-1).long()].repeat_interleave(S, 0)
    sun = []
    with torch.no_grad():
        for k in range(5):
            out = ref_cpu.field(p, d, xyz, torch.tensor(DIRS5[k]).expand(xyz.shape[0], 3), labels, t_emb).view(N, S, -1)
            _, _, w, _ = ref_cpu.composite(out, z, None, 0.0)
            sun.append(torch.sum(w * out[..., 4], -1).numpy())
    sep = min_separation(sun)
    print(case, width, f"min pairwise separation {sep:.3e}")
    assert sep >= SEPARATION * FP32_RTOL and sep >= SEPARATION * BF16_TOL["sun"], sep
    assert sep >= 1.25 * SEPARATION * BF16_TOL["sun"], sep      # headroom: the GPU tests draw their depths


def test_restatement_pieces():
    g = np.random.default_rng(0)
    p = {"sun_v_net.0.weight": g.standard_normal((4, 9)), "sun_v_net.0.bias": g.standard_normal(4)}
    F, dirs = g.standard_normal((5, 6)), g.standard_normal((2, 3))
    full = np.concatenate([F, np.broadcast_to(dirs[1], (5, 3))], 1) @ p["sun_v_net.0.weight"].T + p["sun_v_net.0.bias"]
    np.testing.assert_allclose(rn.base_preactivation(p, F) + rn.direction_vectors(p, dirs, 6)[1], full, rtol=1e-13)
    w, alb = g.uniform(size=(3, 4)), g.uniform(size=(3, 4, 3))
    rgb, sun, sky = rn.relight_sums(w, alb, np.ones((2, 3, 4)), g.uniform(size=(2, 3)))
    np.testing.assert_allclose(rgb[0], np.clip(np.sum(w[..., None] * alb, -2), 0, 1), rtol=1e-13)   # full sun: the albedo
    np.testing.assert_allclose(sun[1], w.sum(-1), rtol=1e-13)
