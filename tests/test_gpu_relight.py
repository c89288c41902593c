"""``relight_image`` on the GPU (csrc/relight.hip, spnerf_amd.relight) — needs an MI355X.

The oracle everywhere is ``render_image`` with the rays' sun columns replaced, one call per
direction, under the same ``PhiloxRandom`` source (whose draws repeat per call).

The modified weights, the five directions and the tolerances are those of tests/relight_cases.py,
which says how they were chosen; tests/test_relight_ref.py checks the choice on the CPU.  Here the
assertion stays on the oracle's own ``sun`` planes: they differ pairwise by at least 20x the
tolerance the test applies — 1e-4 in the fp32 tests, the bf16 ``sun`` bound in the bf16 tests.

fp32 is held to the project's fp32 bound.  bf16 ``relight_image`` is held, per plane, against the
fp32 oracle to twice the norm-relative error that bf16 ``render_image`` shows against that oracle on
these modified weights, rounded up to one digit (relight_cases.BF16_TOL, the measurements beside it).
"""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import golden_util as gu
import spnerf_amd
import view_numpy as vn
from spnerf_amd import PhiloxRandom, random_source
from relight_cases import BF16_TOL, DIRS, SEPARATION, SUN_SCALE, min_separation
from test_gpu_parity import DEV, make_model

pytestmark = pytest.mark.gpu

SUN = ("rgb", "sun", "sky")


@functools.lru_cache(maxsize=None)
def scene(case="a", precision="fp32", width=64, n_samples=None, fixture="view"):
    """(models, args, rays, ts, semantics) of a fixture case with the sun columns scaled."""
    d = vn.load_case(case) if fixture == "view" else gu.load(fixture)
    meta = d["meta"]
    dims, args = gu.dims_of(meta), gu.args_of(meta)
    if width != dims.width:
        dims = dataclasses.replace(dims, width=width)
    if n_samples is not None:
        args.n_samples = n_samples
    models = {"coarse": make_model(dims, meta["seed"], precision)}
    if args.n_importance > 0:
        models["fine"] = make_model(dims, meta["seed"] + 100, precision)
    for m in models.values():
        with torch.no_grad():
            m.sun_v_net[0].weight[:, dims.width:] *= SUN_SCALE
    ts = None
    if "in_t_embedding" in d:
        emb = torch.nn.Embedding(*d["in_t_embedding"].shape).to(DEV)
        with torch.no_grad():
            emb.weight.copy_(torch.tensor(d["in_t_embedding"]))
        models["t"] = emb
        ts = torch.tensor(d["in_ts"], device=DEV)
    sem = torch.tensor(d["in_semantics"], device=DEV) if "in_semantics" in d else None
    return models, args, torch.tensor(d["rays"], device=DEV), ts, sem


def oracle_planes(sc, dirs, products, seed=5, **kw):
    """render_image with the sun columns replaced, one call per direction: name -> (K, N, ...)."""
    models, args, rays, ts, sem = sc
    res = {p: [] for p in products}
    for d in dirs:
        lit = rays.clone()
        lit[:, 8:11] = torch.tensor(d, device=DEV)
        with random_source(PhiloxRandom(seed)):
            img = spnerf_amd.render_image(models, args, lit, ts, sem, products=products, **kw)
        for p in products:
            res[p].append(img[p].cpu().numpy())
    return {p: np.stack(v) for p, v in res.items()}


@functools.lru_cache(maxsize=None)
def oracle_case(case, width, precision="fp32", n_samples=None):
    return oracle_planes(scene(case, precision, width, n_samples), DIRS, SUN)


def relight(sc, dirs, products=SUN, seed=5, **kw):
    models, args, rays, ts, sem = sc
    with random_source(PhiloxRandom(seed)):
        return spnerf_amd.relight_image(models, args, rays, torch.tensor(np.asarray(dirs)), ts, sem, products=products, **kw)


def assert_directions_matter(ref_sun, tol):
    """The oracle's sun planes differ pairwise by at least 20x the tolerance in use (norm-relative)."""
    sep = min_separation(ref_sun)
    assert sep >= SEPARATION * tol, (sep, tol)


@pytest.mark.parametrize("width", [64, 256])
@pytest.mark.parametrize("case", vn.CASES)
def test_fp32_matches_render_image_per_direction(case, width):
    sc = scene(case, "fp32", width)
    ref = oracle_case(case, width)
    assert_directions_matter(ref["sun"], 1e-4)
    got = relight(sc, DIRS)
    assert sorted(got) == sorted(SUN) and got["rgb"].shape == (5, 120, 3) and got["sun"].shape == (5, 120)
    for p in SUN:
        print(case, width, p, f"{gu.rel_err(got[p].cpu().numpy(), ref[p]):.2e}")
        gu.assert_close(f"{case}:w{width}:{p}", got[p].cpu().numpy(), ref[p], rtol=1e-4, atol_frac=1e-5)
    # K = 1 with the rays' own direction: render_image on the rays as they are
    models, args, rays, ts, sem = sc
    own = rays[0, 8:11].cpu().numpy()
    assert bool((rays[:, 8:11] == rays[0, 8:11]).all())
    one = relight(sc, own[None])
    with random_source(PhiloxRandom(5)):
        img = spnerf_amd.render_image(models, args, rays, ts, sem, products=SUN)
    for p in SUN:
        gu.assert_close(f"{case}:w{width}:own:{p}", one[p][0].cpu().numpy(), img[p].cpu().numpy(), rtol=1e-4, atol_frac=1e-5)


@pytest.mark.parametrize("width", [64, 256])
@pytest.mark.parametrize("case", vn.CASES)
def test_bf16_within_twice_render_images_own_error(case, width):
    ref = oracle_case(case, width)
    assert_directions_matter(ref["sun"], BF16_TOL["sun"])
    base = oracle_case(case, width, "bf16")     # existing code on both sides: the measurement
    got = relight(scene(case, "bf16", width), DIRS)
    for p in SUN:
        err = gu.rel_err(got[p].cpu().numpy(), ref[p])
        print(case, width, p, f"render_image bf16 {gu.rel_err(base[p], ref[p]):.2e}  relight_image bf16 {err:.2e}")
        assert err <= BF16_TOL[p], (case, width, p, err)


@pytest.mark.parametrize("precision,width", [("fp32", 64), ("bf16", 64), ("bf16", 256)])
def test_plane_k_depends_neither_on_K_nor_on_its_position(precision, width):
    sc = scene("b", precision, width)
    five = relight(sc, DIRS)
    for k in range(5):
        one = relight(sc, DIRS[k:k + 1])
        for p in SUN:
            assert torch.equal(five[p][k], one[p][0]), (p, k)
    perm = [3, 0, 4, 2, 1]
    moved = relight(sc, DIRS[perm])
    for p in SUN:
        assert torch.equal(moved[p], five[p][perm]), p


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_chunking_leaves_every_bit(precision):
    """chunk=50 splits the 120 rays into 50 / 50 / 20; with on-device draws and σ noise on."""
    models, args, rays, ts, sem = scene("c", precision)
    args = type(args)(**vars(args))
    args.noise_std = 0.37
    sc = (models, args, rays, ts, sem)
    prod = SUN + ("depth", "albedo", "sem") + (("beta",) if models["coarse"].beta else ())
    whole = relight(sc, DIRS, prod)
    parts = relight(sc, DIRS, prod, chunk=50)
    assert sorted(whole) == sorted(parts)
    for p in whole:
        assert torch.equal(whole[p], parts[p]), p
    if precision == "fp32":   # the K planes and the geometry share the oracle's σ-noise draw
        ref = oracle_planes(sc, DIRS[:2], ("rgb", "sun", "depth"))
        gu.assert_close("noise rgb", whole["rgb"][:2].cpu().numpy(), ref["rgb"], rtol=1e-4, atol_frac=1e-5)
        gu.assert_close("noise sun", whole["sun"][:2].cpu().numpy(), ref["sun"], rtol=1e-4, atol_frac=1e-5)
        assert np.array_equal(whole["depth"].cpu().numpy(), ref["depth"][0])


@pytest.mark.parametrize("n_samples", [33, 65])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_rays_straddling_128_point_tiles(n_samples, precision):
    ref = oracle_case("a", 64, "fp32", n_samples)
    got = relight(scene("a", precision, 64, n_samples), DIRS)
    for p in SUN:
        if precision == "fp32":
            gu.assert_close(f"S{n_samples}:{p}", got[p].cpu().numpy(), ref[p], rtol=1e-4, atol_frac=1e-5)
        else:
            assert gu.rel_err(got[p].cpu().numpy(), ref[p]) <= BF16_TOL[p], (p, gu.rel_err(got[p].cpu().numpy(), ref[p]))


def test_sun_independent_products_come_back_once():
    sc = scene("c", "fp32")
    models, args, rays, ts, sem = sc
    prod = ("depth", "albedo", "sem") + (("beta",) if models["coarse"].beta else ())
    got = relight(sc, DIRS[:2], SUN + prod)
    with random_source(PhiloxRandom(5)):
        img = spnerf_amd.render_image(models, args, rays, ts, sem, products=prod)
    assert sorted(got) == sorted(list(SUN) + list(img))
    for p in img:
        assert got[p].shape == img[p].shape and torch.equal(got[p], img[p]), p


def test_out_planes_of_a_larger_image():
    sc = scene("a", "bf16")
    ref = relight(sc, DIRS[:3], SUN + ("depth",), ray_offset=6)   # the draws are keyed by ray_offset + i
    out = {"rgb": torch.full((3, 130, 3), -7.0, device=DEV), "sun": torch.full((3, 130), -7.0, device=DEV),
           "sky": torch.full((3, 130, 3), -7.0, device=DEV), "depth": torch.full((130,), -7.0, device=DEV)}
    models, args, rays, ts, sem = sc
    with random_source(PhiloxRandom(5, ray_offset=0)):
        res = spnerf_amd.relight_image(models, args, rays, torch.tensor(DIRS[:3]), ts, sem, products=SUN + ("depth",), out=out,
                                       ray_offset=6)
    assert res["rgb"] is out["rgb"]
    for p in SUN:
        assert bool((out[p][:, :6] == -7).all()) and bool((out[p][:, 126:] == -7).all()), p
        assert torch.equal(out[p][:, 6:126], ref[p]), p          # every direction's window, bit for bit
    assert torch.equal(out["depth"][6:126], ref["depth"])
    assert bool((out["depth"][:6] == -7).all()) and bool((out["depth"][126:] == -7).all())
    # the same shard rendered by the oracle at that offset
    lit = rays.clone()
    lit[:, 8:11] = torch.tensor(DIRS[1], device=DEV)
    big = {"rgb": torch.zeros(130, 3, device=DEV)}
    with random_source(PhiloxRandom(5)):
        spnerf_amd.render_image(models, args, lit, ts, sem, products=("rgb",), out=big, ray_offset=6)
    assert gu.rel_err(out["rgb"][1, 6:126].cpu().numpy(), big["rgb"][6:126].cpu().numpy()) <= BF16_TOL["rgb"]


def test_fine_model_planes():
    sc = scene(fixture="fine_w64")
    assert sc[1].n_importance > 0
    ref = oracle_planes(sc, DIRS[:2], SUN + ("rgb_coarse", "depth"))
    got = relight(sc, DIRS[:2], SUN + ("rgb_coarse", "depth"))
    for p in SUN:
        gu.assert_close(f"fine:{p}", got[p].cpu().numpy(), ref[p], rtol=1e-4, atol_frac=1e-5)
    assert np.array_equal(got["depth"].cpu().numpy(), ref["depth"][0])
    # the coarse image is sun-independent output: the coarse model's under the rays' own sun columns
    models, args, rays, ts, sem = sc
    with random_source(PhiloxRandom(5)):
        own = spnerf_amd.render_image(models, args, rays, ts, sem, products=("rgb", "rgb_coarse"))
    assert torch.equal(got["rgb_coarse"], own["rgb_coarse"])


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_guided_sampling_merges_the_two_forwards(precision):
    models, args, rays, ts, sem = scene("a", precision)
    args = type(args)(**vars(args))
    args.guidedsample, args.n_samples = True, 24
    sc = (models, args, rays, ts, sem)
    ref = oracle_planes((scene("a", "fp32")[0],) + sc[1:], DIRS[:2], SUN)
    got = relight(sc, DIRS[:2])
    for p in SUN:
        if precision == "fp32":
            gu.assert_close(f"guided:{p}", got[p].cpu().numpy(), ref[p], rtol=1e-4, atol_frac=1e-5)
        else:
            assert gu.rel_err(got[p].cpu().numpy(), ref[p]) <= BF16_TOL[p], p


def test_more_than_32_directions_run_in_groups():
    """K = 35: two passes over the geometry (32 + 3 directions); every plane is its K = 1 call's."""
    from spnerf_amd.relight import MAX_DIRS_PER_PASS
    assert MAX_DIRS_PER_PASS == 32
    sc = scene("b", "bf16")
    many = np.concatenate([DIRS] * 7)
    many[31], many[32] = DIRS[1], DIRS[4]
    got = relight(sc, many, SUN + ("depth",))
    assert got["rgb"].shape == (35, 120, 3) and got["sun"].shape == (35, 120) and got["depth"].shape == (120,)
    five = relight(sc, DIRS, SUN + ("depth",))
    for p in SUN:
        for k in (0, 31, 32, 34):
            j = {31: 1, 32: 4}.get(k, k % 5)
            assert torch.equal(got[p][k], five[p][j]), (p, k)
    assert torch.equal(got["depth"], five["depth"])


def test_width_512_falls_back_to_the_definition():
    sc = scene("a", "bf16", 512)
    ref = oracle_planes(sc, DIRS[:2], SUN + ("depth",))
    got = relight(sc, DIRS[:2], SUN + ("depth",))
    for p in SUN:
        assert np.array_equal(got[p].cpu().numpy(), ref[p]), p
    assert np.array_equal(got["depth"].cpu().numpy(), ref["depth"][0])


def test_sc_is_refused():
    models, args, rays, ts, sem = scene("a")
    with pytest.raises(ValueError, match="sc product"):
        spnerf_amd.relight_image(models, args, rays, torch.tensor(DIRS), ts, sem, products=("sc",))
