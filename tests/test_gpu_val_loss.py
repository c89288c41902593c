"""The validation loss of whole views on the GPU (csrc/val.hip, spnerf_amd.view: the "sc" and
"rgb_coarse" products, ``view_loss``, ``view_metrics(loss=)``) — needs an MI355X; fp32.

  * parity: ``render_image(products=(..., "sc"))`` + ``view_loss`` on the cases of
    tests/golden/val_loss.npz against what the reference's render_rays and SNerfLoss / SatNerfLoss
    computed, at the tolerance tests/test_gpu_view.py applies to render_image's planes (1e-4
    relative, floor 1e-5 of the plane's largest value; 1e-4 for what the fine pass derives), every
    recorded draw consumed;
  * the march is the composite's: the planes equal ``render_rays``' per-sample solar tensors reduced
    in the kernel's own order restated in torch, bit for bit;
  * ``spnerf_val_solar_terms`` directly on synthetic rows (opaque and empty rays, S around the lane
    count, a ragged block, ray_begin) against the fp64 restatement tests/val_loss_numpy.py, within
    the worst-case error of an fp32 sum of S rounded products, (S + 3) · 2^-24 · Σ|terms|;
  * chunk and shard independence with on-device draws; the fp64 reduction against numpy; the
    defaults of render_image and view_metrics unchanged.
"""
import functools
import types

import numpy as np
import pytest
import torch

import golden_util as gu
import spnerf_amd
import val_loss_numpy as vl
from spnerf_amd import PhiloxRandom, ReplayRandom, _lib, _val_lib, random_source
from spnerf_amd.spnerf import _Composite
from oracle.weights import ModelDims
from test_gpu_parity import DEV, make_model

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24


def scene(case):
    """(fixture, args, models, rays, ts, semantics, target) of a fixture case on the device."""
    d = vl.load_case(case)
    meta = d["meta"]
    dims, args = gu.dims_of(meta), gu.args_of(meta)
    models = {"coarse": make_model(dims, meta["seed"])}
    if args.n_importance > 0:
        models["fine"] = make_model(dims, meta["seed"] + 100)
    ts = None
    if "in_t_embedding" in d:
        emb = torch.nn.Embedding(*d["in_t_embedding"].shape).to(DEV)
        with torch.no_grad():
            emb.weight.copy_(torch.tensor(d["in_t_embedding"]))
        models["t"] = emb
        ts = torch.tensor(d["in_ts"], device=DEV)
    sems = torch.tensor(d["in_semantics"], device=DEV) if "in_semantics" in d else None
    return d, args, models, torch.tensor(d["rays"], device=DEV), ts, sems, torch.tensor(d["target"], device=DEV)


@functools.lru_cache(maxsize=None)
def render_case(case):
    """(fixture, planes on the device, view_loss) of a solar case, rendered once."""
    d, args, models, rays, ts, sems, target = scene(case)
    beta = d["meta"]["dims"]["beta"]
    products = ("rgb", "depth") + (("beta",) if beta else ()) + ("sc",)
    with random_source(ReplayRandom(gu.draws_of(d))) as src:
        planes = spnerf_amd.render_image(models, args, rays, ts, sems, products=products)
    assert src.used == len(src.draws), "random draws consumed differ from the reference's validation step"
    loss = spnerf_amd.view_loss(planes, target, args.sc_lambda, beta=beta)
    return d, planes, loss


def close_scalars(name, got: dict, ref: dict, atol_frac=1e-5):
    assert sorted(got) == sorted(ref), (name, sorted(got), sorted(ref))
    for k, v in ref.items():
        print(name, k, got[k], v, f"rel {abs(got[k] - v) / abs(v):.2e}")
        gu.assert_close(f"{name}:{k}", np.array([got[k]]), np.array([v]), rtol=1e-4, atol_frac=atol_frac)


# ---- 1. the fixture's solar cases ------------------------------------------------------------------

@pytest.mark.parametrize("case", vl.SOLAR_CASES)
def test_solar_planes_and_loss_match_reference(case):
    d, planes, loss = render_case(case)
    n = d["meta"]["n_rays"]
    beta = d["meta"]["dims"]["beta"]
    assert sorted(planes) == sorted(["rgb", "depth", "sc_term2", "sc_term3"] + ["beta"] * beta)
    ref = vl.reference_planes(d)
    for k, r in (("sc_term2", ref["term2"]), ("sc_term3", ref["term3"]), ("rgb", d["out_rgb_coarse"]), ("depth", d["out_depth_coarse"])):
        got = planes[k].cpu().numpy()
        assert got.dtype == np.float32 and got.shape == ((n, 3) if k == "rgb" else (n,))
        print(case, k, f"{gu.rel_err(got, r):.2e}")
        gu.assert_close(f"{case}:{k}", got, r, rtol=1e-4, atol_frac=1e-5)
    if beta:
        gu.assert_close(f"{case}:beta", planes["beta"].cpu().numpy(), d["sum_beta"], rtol=1e-4, atol_frac=1e-5)
    close_scalars(case, loss, dict(d["terms"], loss=d["loss"]))
    # and the restatement on the library's own planes: the fp64 reduction adds nothing to that error
    a = d["meta"]["args"]
    own = vl.view_loss(planes["rgb"].cpu().numpy(), d["target"], a["sc_lambda"], planes["sc_term2"].cpu().numpy(),
                       planes["sc_term3"].cpu().numpy(), planes["beta"].cpu().numpy() if beta else None)
    for k, v in own.items():
        assert abs(loss[k] - v) <= 1e-10 * abs(v), (k, loss[k], v)


# ---- 2. the coarse image beside a fine model's -------------------------------------------------------

def test_rgb_coarse_and_the_two_colour_terms():
    d, args, models, rays, ts, sems, target = scene("e")
    with random_source(ReplayRandom(gu.draws_of(d))) as src:
        planes = spnerf_amd.render_image(models, args, rays, ts, sems, products=("rgb", "depth", "rgb_coarse"))
    assert src.used == len(src.draws)
    with random_source(ReplayRandom(gu.draws_of(d))) as src0:
        plain = spnerf_amd.render_image(models, args, rays, ts, sems, products=("rgb", "depth"))
    assert src0.used == len(src0.draws)
    assert sorted(planes) == ["depth", "rgb", "rgb_coarse"] and sorted(plain) == ["depth", "rgb"]
    assert torch.equal(planes["rgb"], plain["rgb"]) and torch.equal(planes["depth"], plain["depth"])
    gu.assert_close("e:rgb_coarse", planes["rgb_coarse"].cpu().numpy(), d["out_rgb_coarse"], rtol=1e-4, atol_frac=1e-5)
    # downstream of the fine pass: the floor test_gpu_view.py gives the fine fixture's rgb
    gu.assert_close("e:rgb", planes["rgb"].cpu().numpy(), d["out_rgb_fine"], rtol=1e-4, atol_frac=1e-4)
    loss = spnerf_amd.view_loss(planes, target, args.sc_lambda)
    close_scalars("e", {k: loss[k] for k in ("coarse_color",)}, {"coarse_color": d["terms"]["coarse_color"]})
    close_scalars("e", loss, dict(d["terms"], loss=d["loss"]), atol_frac=1e-4)
    # shards of the coarse image go where the others go
    out = {k: torch.full((40,) + tuple(v.shape[1:]), -7.0, device=DEV) for k, v in planes.items()}
    with random_source(ReplayRandom(gu.draws_of(d))):
        spnerf_amd.render_image(models, args, rays, ts, sems, products=("rgb", "depth", "rgb_coarse"), out=out, ray_offset=2)
    assert torch.equal(out["rgb_coarse"][2:39], planes["rgb_coarse"])
    assert bool((out["rgb_coarse"][:2] == -7).all()) and bool((out["rgb_coarse"][39:] == -7).all())
    with pytest.raises(ValueError, match="per sample"):
        spnerf_amd.view_loss(dict(planes, beta=planes["depth"]), target, 0.0, beta=True)


# ---- 3. the same bits as the per-sample path ---------------------------------------------------------

def kernel_order_sum(p):
    """Σ over the samples of a (B, S) fp32 tensor in k_val_solar_terms' order: lane l adds its EPL
    consecutive samples in index order from 0, then the xor butterfly (32, 16, ..., 1) adds the lanes."""
    B, S = p.shape
    epl = 1 if S <= 64 else (2 if S <= 128 else 4)
    v = torch.zeros(B, 64 * epl, dtype=torch.float32, device=p.device)
    v[:, :S] = p
    v = v.view(B, 64, epl)
    acc = torch.zeros(B, 64, dtype=torch.float32, device=p.device)
    for j in range(epl):
        acc = acc + v[:, :, j]
    lanes = torch.arange(64, device=p.device)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ off]
    return acc[:, 0]


def kernel_order_terms(T, w, sun):
    d = T - sun
    return kernel_order_sum(d * d), 1.0 - kernel_order_sum(w * sun)


def test_planes_are_the_per_sample_solar_pass_reduced():
    d, planes, _ = render_case("c")
    _, args, models, rays, ts, sems, _ = scene("c")
    with random_source(ReplayRandom(gu.draws_of(d))), torch.no_grad():
        res = spnerf_amd.render_rays(models, args, rays, ts, semantics=sems, mode="test")
    T, w, sun = res["transparency_sc_coarse"], res["weights_sc_coarse"], res["sun_sc_coarse"].reshape(37, 96)
    t2, t3 = kernel_order_terms(T, w, sun)
    assert torch.equal(planes["sc_term2"], t2) and torch.equal(planes["sc_term3"], t3)
    assert torch.equal(planes["rgb"], res["rgb_coarse"]) and torch.equal(planes["depth"], res["depth_coarse"])


# ---- 4. the kernel on synthetic rows -----------------------------------------------------------------

def solar_direct(out, z, noise, std, n_total, begin, sun_col=4, fill=-7.0):
    B, S = z.shape
    t2 = torch.full((n_total,), fill, device=DEV)
    t3 = torch.full((n_total,), fill, device=DEV)
    _lib.check(_val_lib.lib().spnerf_val_solar_terms(B, S, _lib.ptr(z), _lib.ptr(out), out.shape[1], sun_col, _lib.ptr(noise),
                                                     float(std), begin, _lib.ptr(t2), _lib.ptr(t3), None,
                                                     _lib.stream_of(out)), "val_solar_terms")
    return t2, t3


def synthetic_rows(B, S, NO, seed):
    """Rows of a sun-only forward: σ in column 3, sun in column 4; ray 0 opaque (σ = 1e4 at the first
    sample), ray 1 empty (σ = 0 everywhere)."""
    g = np.random.default_rng(seed)
    raw = g.uniform(0, 1, (B, S, NO)).astype(np.float32)
    raw[..., 3] = g.exponential(2.0, (B, S)) * g.choice([1e-2, 1.0, 50.0], (B, 1))
    raw[0, 0, 3] = 1e4
    raw[1, :, 3] = 0.0
    z = (0.01 * np.arange(S, dtype=np.float32)[None] + np.sort(g.uniform(0, 0.005, (B, S)).astype(np.float32), -1))
    noise = g.standard_normal((B, S)).astype(np.float32)
    noise[:2] = 0.0
    return raw, z, noise


@pytest.mark.parametrize("S", [1, 63, 64, 65, 128])
@pytest.mark.parametrize("begin", [0, 3])
def test_solar_terms_kernel_edges(S, begin):
    B, NO, std = 5, 9, 0.3                      # 5 rays: not a multiple of the 4 waves of a block
    raw, z, noise = synthetic_rows(B, S, NO, seed=S)
    out, zt, nt = torch.tensor(raw.reshape(B * S, NO), device=DEV), torch.tensor(z, device=DEV), torch.tensor(noise, device=DEV)
    t2, t3 = solar_direct(out, zt, nt, std, B + begin + 4, begin)
    sl = slice(begin, begin + B)
    for t in (t2, t3):                          # the rest of the larger plane keeps the sentinel
        assert bool((t[:begin] == -7).all()) and bool((t[begin + B:] == -7).all())
    # the composite's own T and w on these rows: the same march, so the kernel's order restated is exact
    sun, _, w, T, _ = _Composite.apply(out, zt, nt, std, 8, 0, True, None, None, True)
    k2, k3 = kernel_order_terms(T, w, sun)
    assert torch.equal(t2[sl], k2) and torch.equal(t3[sl], k3)
    # and the fp64 formulas on them, within the error of an fp32 sum of S rounded products
    r2, r3 = vl.solar_terms(T.cpu().numpy(), w.cpu().numpy(), sun.cpu().numpy())
    Td, wd, sd = (x.double().cpu().numpy() for x in (T, w, sun))
    b2 = (S + 3) * EPS * np.sum((Td - sd) ** 2, -1)
    b3 = (S + 3) * EPS * (1.0 + np.sum(wd * sd, -1))
    e2, e3 = np.abs(t2[sl].double().cpu().numpy() - r2), np.abs(t3[sl].double().cpu().numpy() - r3)
    print(S, "worst err / bound", float((e2 / b2).max()), float((e3 / b3).max()))
    assert (e2 <= b2).all() and (e3 <= b3).all()
    # the opaque and the empty ray against the fp64 march of the rows themselves: T differs from it
    # by at most S · 1e-9 there (empty: fp32 rounds 1 + 1e-10 to 1; opaque: T <= 1e-10 · (1 + 2^-24)
    # after the first sample)
    Tm, wm = vl.march(raw[:2, :, 3], z[:2])
    m2, m3 = vl.solar_terms(Tm, wm, raw[:2, :, 4])
    got2, got3 = t2[sl][:2].double().cpu().numpy(), t3[sl][:2].double().cpu().numpy()
    assert (np.abs(got2 - m2) <= b2[:2] + 2 * S * 1e-9 * S).all(), (got2, m2)
    assert (np.abs(got3 - m3) <= b3[:2] + S * 1e-9).all(), (got3, m3)
    sun0 = raw[:2, :, 4].astype(np.float64)
    assert abs(got3[1] - 1.0) <= EPS                                           # empty: no weight anywhere
    assert abs(got2[1] - np.sum((1.0 - sun0[1]) ** 2)) <= b2[1] + 2 * S * S * 1e-9
    assert abs(got3[0] - (1.0 - sun0[0, 0])) <= b3[0] + S * 1e-9                # opaque: all the weight on sample 0
    # another sun column of the same rows, no noise
    u2, u3 = solar_direct(out, zt, None, 0.0, B, 0, sun_col=6)
    sun6 = out.view(B, S, NO)[..., 6].contiguous()
    _, _, w0, T0, _ = _Composite.apply(out, zt, None, 0.0, 8, 0, True)
    k2, k3 = kernel_order_terms(T0, w0, sun6)
    assert torch.equal(u2, k2) and torch.equal(u3, k3)


# ---- 5. chunks and shards ----------------------------------------------------------------------------

def test_solar_planes_do_not_depend_on_chunking_or_sharding():
    dims = ModelDims(width=64, sem=True)
    args = gu.args_of({"args": dict(n_samples=16, n_importance=0, model="sp-nerf", beta=False, guidedsample=True,
                                    sc_lambda=0.1, margin=1e-4, stdscale=1.0, chunk=5120, noise_std=0.1)})
    models = {"coarse": make_model(dims, 3)}
    n = 50
    rays = torch.tensor(gu.synthetic_rays(n, seed=78), device=DEV)
    sems = torch.tensor(np.random.default_rng(1).choice([0, 1, 2, -100], size=n), device=DEV)
    products = ("rgb", "depth", "sem", "sc")
    images = []
    for chunk in (n, 7):
        with random_source(PhiloxRandom(seed=5)):
            images.append(spnerf_amd.render_image(models, args, rays, None, sems, chunk=chunk, products=products))
    whole = images[0]
    assert sorted(whole) == ["depth", "rgb", "sc_term2", "sc_term3", "sem_class", "sem_logits"]
    for k, v in whole.items():
        assert torch.equal(v, images[1][k]), k
    assert float(whole["sc_term2"].min()) > 0 and not torch.equal(whole["sc_term2"], whole["sc_term3"])
    out = {k: torch.full_like(v, -7) for k, v in whole.items()}
    with random_source(PhiloxRandom(seed=5)):
        for i0, i1 in ((0, 23), (23, n)):
            spnerf_amd.render_image(models, args, rays[i0:i1], None, sems[i0:i1], products=products, out=out, ray_offset=i0,
                                    clamp_near_far=rays[0, 6:8])
    for k, v in whole.items():
        assert torch.equal(v, out[k]), k
    # with the draws on, the solar pass's noise is a slot of its own: another seed moves the terms
    with random_source(PhiloxRandom(seed=6)):
        other = spnerf_amd.render_image(models, args, rays, None, sems, products=products)
    assert not torch.equal(other["sc_term3"], whole["sc_term3"])


# ---- 6. the reduction --------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 257, 70001])
def test_val_loss_reduction_matches_numpy(n):
    g = np.random.default_rng(n)
    rgb = g.uniform(0, 1, (n, 3)).astype(np.float32)
    tgt = np.clip(rgb + 0.1 * g.standard_normal((n, 3)), 0, 1).astype(np.float32)
    coarse = np.clip(rgb + 0.2 * g.standard_normal((n, 3)), 0, 1).astype(np.float32)
    beta = g.uniform(0.01, 0.5, n).astype(np.float32)      # log(beta + 0.05) < 0 on every ray: same-signed sums
    t2 = g.uniform(0, 40, n).astype(np.float32)
    t3 = g.uniform(0, 1, n).astype(np.float32)
    dev = lambda a: torch.tensor(a, device=DEV)   # noqa: E731
    target = dev(tgt)
    sat = {"rgb": dev(rgb), "beta": dev(beta), "sc_term2": dev(t2), "sc_term3": dev(t3)}
    fine = {"rgb": dev(rgb), "rgb_coarse": dev(coarse)}
    for name, planes, kw, ref in (
            ("snerf", sat, dict(lambda_sc=0.1), vl.view_loss(rgb, tgt, 0.1, t2, t3)),
            ("satnerf", sat, dict(lambda_sc=0.05, beta=True, beta_min=0.05), vl.view_loss(rgb, tgt, 0.05, t2, t3, beta, 0.05)),
            ("plain", sat, dict(lambda_sc=0.0), vl.view_loss(rgb, tgt)),
            ("fine", fine, dict(lambda_sc=0.0), vl.view_loss(rgb, tgt, rgb_coarse=coarse))):
        got = spnerf_amd.view_loss(planes, target, **kw)
        assert sorted(got) == sorted(ref), (name, sorted(got))
        for k, v in ref.items():
            assert abs(got[k] - v) <= 1e-10 * abs(v), (name, k, got[k], v)
        assert spnerf_amd.view_loss(planes, target, **kw) == got                   # two calls, equal bits
        plain = spnerf_amd.view_metrics(planes, target)
        both = spnerf_amd.view_metrics(planes, target, loss=kw)
        assert {k: both[k] for k in got} == got
        assert sorted(set(both) - set(got)) == sorted(plain) and all(both[k] == plain[k] for k in plain)


def test_view_loss_refuses_missing_planes():
    rgb = torch.zeros(4, 3, device=DEV)
    with pytest.raises(ValueError, match="sc_term2"):
        spnerf_amd.view_loss({"rgb": rgb}, rgb, 0.1)
    with pytest.raises(ValueError, match="'beta'"):
        spnerf_amd.view_loss({"rgb": rgb}, rgb, 0.0, beta=True)
    with pytest.raises(ValueError, match="dictionary"):
        spnerf_amd.view_metrics(rgb, rgb, loss=dict(lambda_sc=0.0))
    with pytest.raises(ValueError, match="not the target's"):
        spnerf_amd.view_loss({"rgb": torch.zeros(5, 3, device=DEV)}, rgb, 0.0)


# ---- 7. the defaults stay what they were -------------------------------------------------------------

def profiled(fn):
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        res = fn()
        torch.cuda.synchronize()
    finally:
        _lib.prof_enable(False)
    return res, {c: _lib.prof_read(c)["launches"] for c in _lib.prof_classes()}


def test_defaults_render_and_score_as_before():
    d, args, models, rays, ts, sems, target = scene("a")
    assert args.sc_lambda == 0.1
    with random_source(ReplayRandom(gu.draws_of(d))) as src:
        planes, launched = profiled(lambda: spnerf_amd.render_image(models, args, rays, ts, sems))
    # "sc_lambda taken as 0": the solar pass's noise, the last recorded draw, is left over
    left = src.draws[src.used:]
    assert len(left) == 1 and left[0][0] == "randn" and np.array_equal(left[0][1], d["rng04_randn"])
    assert "val_solar_terms" not in launched and launched["composite_products"] == 1
    zero = types.SimpleNamespace(**dict(vars(args), sc_lambda=0.0))
    with random_source(ReplayRandom(gu.draws_of(d)[:-1])) as src0:
        same = spnerf_amd.render_image(models, zero, rays, ts, sems)
    assert src0.used == len(src0.draws)
    assert sorted(planes) == sorted(same) == ["albedo", "depth", "rgb", "sem_class", "sem_logits", "sky", "sun"]
    for k, v in same.items():
        assert torch.equal(planes[k], v), k
    # with the product: one launch of the solar terms per chunk, the other planes untouched
    with random_source(ReplayRandom(gu.draws_of(d))):
        sc, launched = profiled(lambda: spnerf_amd.render_image(models, args, rays, ts, sems, products=("rgb", "depth", "sc")))
    assert launched["val_solar_terms"] == 1 == launched["composite_products"]
    assert torch.equal(sc["rgb"], planes["rgb"]) and torch.equal(sc["depth"], planes["depth"])
    # the metrics without loss= launch what they launched; with it, one more class
    _, launched = profiled(lambda: spnerf_amd.view_metrics(planes, target))
    assert sorted(launched) == ["view_metrics"] and launched["view_metrics"] == 1
    _, launched = profiled(lambda: spnerf_amd.view_metrics(sc, target, loss=dict(lambda_sc=0.1)))
    assert sorted(launched) == ["val_loss", "view_metrics"] and launched["val_loss"] == 1
