"""The on-device Philox draws (``rng_uniform`` / ``rng_normal``, csrc/common.h) against the numpy
reference oracle/philox_ref.py — needs an MI355X.

  * ``spnerf_rng_fill`` materialises the draws of a key: the uniforms must equal the reference bit
    for bit (a 24-bit integer times 2^-24 is exact), the normals the float64 Box–Muller within a
    derived bound (below);
  * every kernel that consumes draws — stratified, sample_pdf, guided, composite forward and
    backward — run with an ``spnerf_rng`` must give, bit for bit, what the same entry point gives
    when handed the reference's uniforms (or the filled normals) as a buffer: it draws the slot,
    ray id and index it claims;
  * a whole ``render_rays`` under ``PhiloxRandom`` equals, outputs and gradients, the render under
    ``ReplayRandom(philox_ref.render_draws(...))``: every pass takes the slot INTEGRATION.md lists.

The normal's bound: the angle 6.2831853f·u2 rounds to float with error <= ulp(8)/2 = 2.4e-7 and the
fp32 constant adds <= 1.8e-7; the radius is <= sqrt(2·ln 2^24) = 5.77, so the angle contributes
<= 2.4e-6; a few ulp of logf / sqrtf / cosf on values <= 5.77 add <= 2e-6: |Δ| <= 1e-5 absolute.
The same fp32 arithmetic in numpy on the host differs from the float64 reference by at most 1.6e-6
(2^20 draws, seed 7, step 3).  Measured on the MI355X over the cases below: 1.49e-6 at most
(every case prints its own maximum)."""
import numpy as np
import pytest
import torch

import golden_util as gu
import spnerf_amd
from oracle import philox_ref as pr
from spnerf_amd import PhiloxRandom, ReplayRandom, _lib, random_source, rendering
from test_gpu_parity import DEV, make_model

pytestmark = pytest.mark.gpu

NORMAL_TOL = 1e-5
BIG_SEED = 0x1234_5678_9abc_def0
FAR_RAY0 = 2 ** 32 - 100


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV).contiguous()


class Key:
    """An spnerf_rng over a snapshot {seed, step} of its own."""

    def __init__(self, seed, step, ray0=0, slot=0):
        self.seed, self.step, self.ray0, self.slot = seed, step, ray0, slot
        self.snap = torch.tensor([seed, step], dtype=torch.int64, device=DEV)
        self.rng = _lib.Rng(self.snap.data_ptr(), ray0, slot, 0)

    def ref_uniform(self, B, n, slot_offset=0):
        return pr.uniform(self.seed, self.step, self.ray0, B, n, self.slot + slot_offset)

    def fill(self, kind, B, n):
        out = torch.empty(B, n, device=DEV)
        _lib.check(_lib.lib().spnerf_rng_fill(_lib.rng_ref(self.rng), kind, B, n, _lib.ptr(out), _lib.stream_of(out)),
                   "rng_fill")
        return out


def check_fill(src: PhiloxRandom, seed, step, ray0, slot, rays, n):
    u = src.fill("rand", rays, n, slot, DEV).cpu().numpy()
    np.testing.assert_array_equal(u, pr.uniform(seed, step, ray0, rays, n, slot))
    z = src.fill("randn", rays, n, slot, DEV).cpu().numpy()
    err = float(np.abs(z.astype(np.float64) - pr.normal(seed, step, ray0, rays, n, slot)).max())
    print(f"seed {seed:#x} step {step} ray0 {ray0} slot {slot} ({rays} x {n}): max |normal - float64 reference| {err:.3e}")
    assert err <= NORMAL_TOL, err
    return err


# (seed, reset_step argument, ray_offset, slot, rays, n): the render after reset_step(s) is step s + 1
FILL_CASES = {
    "seed0_step0": (0, -1, 0, 0, 257, 130),
    "seed7_step3": (7, 2, 0, 0, 257, 130),
    "seed_high_word": (BIG_SEED, 2, 0, 0, 257, 130),
    "step_high_word": (7, 2 ** 32 + 5, 0, 0, 257, 130),
    "ids_straddle_2^32": (7, 2, FAR_RAY0, 0, 257, 130),
    "slot1": (7, 2, 0, 1, 257, 130),
    "slot7": (7, 2, 0, 7, 257, 130),
    "n65536": (7, 2, 0, 0, 3, 65536),
}


@pytest.mark.parametrize("case", sorted(FILL_CASES))
def test_rng_fill_equals_reference(case):
    seed, reset, ray0, slot, rays, n = FILL_CASES[case]
    src = PhiloxRandom(seed=seed, ray_offset=ray0)
    src.reset_step(reset)
    src.begin_render(DEV)
    check_fill(src, seed, reset + 1, ray0, slot, rays, n)


def test_reset_step_on_a_live_state_and_successive_renders():
    """begin_render advances the step by exactly one, reset_step moves a state that already lives on
    the device, and a render's snapshot keeps its draws when later renders advance the state."""
    src = PhiloxRandom(seed=7)
    src.begin_render(DEV)                      # step 0
    old = _lib.Rng(src._snap.data_ptr(), 0, 0, 0)
    old_snap = src._snap
    check_fill(src, 7, 0, 0, 0, 33, 70)
    src.begin_render(DEV)                      # step 1
    check_fill(src, 7, 1, 0, 0, 33, 70)
    src.begin_render(DEV)                      # step 2
    check_fill(src, 7, 2, 0, 0, 33, 70)
    out = torch.empty(33, 70, device=DEV)
    _lib.check(_lib.lib().spnerf_rng_fill(_lib.rng_ref(old), 0, 33, 70, _lib.ptr(out), _lib.stream_of(out)))
    np.testing.assert_array_equal(out.cpu().numpy(), pr.uniform(7, 0, 0, 33, 70, 0))
    assert old_snap.tolist() == [7, 0]
    src.reset_step(2 ** 32 + 5)
    src.begin_render(DEV)
    check_fill(src, 7, 2 ** 32 + 6, 0, 0, 33, 70)
    assert src.sync_host_step() == 2 ** 32 + 6


def test_rng_fill_arguments():
    L = _lib.lib()
    k = Key(1, 1)
    out = torch.empty(4, device=DEV)
    args = (_lib.ptr(out), _lib.stream_of(out))
    assert L.spnerf_rng_fill(_lib.rng_ref(k.rng), 0, 0, 4, *args) == 0          # empty: OK, no launch
    for kind, rays, n in ((0, 1, 0), (0, 1, 65537), (0, -1, 4), (2, 1, 4)):
        assert L.spnerf_rng_fill(_lib.rng_ref(k.rng), kind, rays, n, *args) == -1, (kind, rays, n)
        assert b"rng_fill" in L.spnerf_last_error()
    assert L.spnerf_rng_fill(_lib.rng_ref(k.rng), 0, 1, 4, None, args[1]) == -1
    assert L.spnerf_rng_fill(None, 0, 1, 4, *args) == -1
    assert L.spnerf_rng_fill(_lib.rng_ref(_lib.Rng(None, 0, 0, 0)), 0, 1, 4, *args) == -1
    torch.cuda.synchronize()


# ---- each consumer draws the slot, ray id and index it claims --------------------------------

KEYS = [(7, 3, 0, 0), (BIG_SEED, 2 ** 32 + 6, FAR_RAY0, 2)]   # (seed, step, ray0, slot)
KEY_IDS = ["ray0=0", "ray0=2^32-100,slot2"]


@pytest.mark.parametrize("key", KEYS, ids=KEY_IDS)
@pytest.mark.parametrize("S", [64, 5])
def test_stratified_draws_its_slot(S, key):
    B = 131
    k = Key(*key)
    rays = dev(gu.synthetic_rays(B, 3))
    L = _lib.lib()

    def run(u, rng):
        z = torch.full((B, S), float("nan"), device=DEV)
        _lib.check(L.spnerf_sample_stratified(B, S, _lib.ptr(rays), rays.stride(0), _lib.ptr(u), _lib.ptr(z),
                                              _lib.rng_ref(rng), _lib.stream_of(z)), "sample_stratified")
        return z

    got, want = run(None, k.rng), run(dev(k.ref_uniform(B, S)), None)
    assert torch.isfinite(want).all() and torch.equal(got, want)


@pytest.mark.parametrize("key", KEYS, ids=KEY_IDS)
@pytest.mark.parametrize("nb,n_imp", [(63, 64), (127, 128), (1, 64)])
def test_sample_pdf_draws_its_slot(nb, n_imp, key):
    B = 7
    k = Key(*key)
    g = np.random.default_rng(nb)
    if nb == 1:   # one bin [0, 1] of weight 1: the CDF is the identity, the samples ARE the draws
        bins, w = np.tile(np.array([0.0, 1.0], np.float32), (B, 1)), np.ones((B, 1), np.float32)
    else:
        bins = np.sort(g.uniform(0.0, 0.2, (B, nb + 1)), -1).astype(np.float32)
        w = g.uniform(0.0, 1.0, (B, nb)).astype(np.float32)
    bins_d, w_d = dev(bins), dev(w)
    L = _lib.lib()

    def run(u, rng):
        out = torch.full((B, n_imp), float("nan"), device=DEV)
        _lib.check(L.spnerf_sample_pdf(B, nb, _lib.ptr(bins_d), _lib.ptr(w_d), n_imp, _lib.ptr(u), 1e-5, _lib.ptr(out),
                                       _lib.rng_ref(rng), _lib.stream_of(out)), "sample_pdf")
        return out

    u = k.ref_uniform(B, n_imp)
    got, want = run(None, k.rng), run(dev(u), None)
    assert torch.isfinite(want).all() and torch.equal(got, want)
    if nb == 1:
        np.testing.assert_array_equal(got.cpu().numpy(), u)


def _guided_inputs(B, n):
    g = np.random.default_rng(n)
    near, far = 0.0, 0.21
    z = np.sort(g.uniform(near, far, (B, n)), -1).astype(np.float32)
    w = g.uniform(0.0, 1.0, (B, n)).astype(np.float32)
    w /= w.sum(-1, keepdims=True)
    depth = (w * z).sum(-1).astype(np.float32)
    valid = (np.arange(B) % 3 != 1).astype(np.int64)        # mixed: both slots within one launch
    tdep = np.stack([g.uniform(0.05, 0.15, B), np.ones(B)], 1).astype(np.float32)
    tstd = g.uniform(0.002, 0.01, B).astype(np.float32)
    return dict(z=dev(z), depth=dev(depth), w=dev(w), nf=dev(np.array([near, far], np.float32)),
                valid=dev(valid, torch.int64), tdep=dev(tdep), tstd=dev(tstd))


@pytest.mark.parametrize("key", KEYS, ids=KEY_IDS)
@pytest.mark.parametrize("train", [True, False], ids=["train", "test"])
@pytest.mark.parametrize("n", [64, 128])
def test_guided_draws_its_two_slots(n, train, key):
    B = 37
    k = Key(*key)
    a = _guided_inputs(B, n)
    L = _lib.lib()

    def run(u_pred, u_gt, rng):
        zs = torch.full((B, 2 * n), float("nan"), device=DEV)
        zu = torch.full((B, 2 * n), float("nan"), device=DEV)
        valid, tdep, tstd = (a["valid"], a["tdep"], a["tstd"]) if train else (None, None, None)
        _lib.check(L.spnerf_sample_guided(B, n, _lib.ptr(a["z"]), _lib.ptr(a["depth"]), _lib.ptr(a["w"]), _lib.ptr(a["nf"]),
                                          _lib.ptr(valid), _lib.ptr(tdep), 2, _lib.ptr(tstd), _lib.ptr(u_pred),
                                          _lib.ptr(u_gt), _lib.ptr(zs), _lib.ptr(zu), _lib.rng_ref(rng),
                                          _lib.stream_of(zs)), "sample_guided")
        return zs, zu

    got = run(None, None, k.rng)
    u_pred, u_gt = dev(k.ref_uniform(B, n)), dev(k.ref_uniform(B, n, 1))   # slot, slot + 1: rows by ray
    want = run(u_pred, u_gt if train else None, None)
    for x, y in zip(got, want):
        assert torch.isfinite(y).all() and torch.equal(x, y)
    if train:   # the two windows really differ: swapping the slots' draws changes the samples
        swapped = run(u_gt, u_pred, None)
        assert not torch.equal(swapped[0], want[0])


@pytest.mark.parametrize("key", KEYS, ids=KEY_IDS)
@pytest.mark.parametrize("weights_only", [False, True], ids=["full", "weights_only"])
@pytest.mark.parametrize("S", [64, 128])
def test_composite_draws_its_slot(S, weights_only, key):
    """forward and backward, noise_std = 1: the on-device σ noise is the filled normal of the same
    key, and sg + noise · noise_std is one expression in both arms, so the results are equal bits."""
    B, NO, n_sem = 37, 11, 3
    k = Key(*key)
    g = np.random.default_rng(S)
    raw = g.uniform(0.0, 1.0, (B * S, NO)).astype(np.float32)
    raw[:, 3] = g.normal(2.0, 3.0, B * S)                    # σ before the noise: both signs
    raw_d = dev(raw)
    z = dev(np.sort(g.uniform(0.0, 0.21, (B, S)), -1).astype(np.float32))
    flags = _lib.SPNERF_COMP_WEIGHTS_ONLY if weights_only else 0
    grads = {n: dev(g.standard_normal(s).astype(np.float32))
             for n, s in (("rgb", (B, 3)), ("depth", (B,)), ("w", (B, S)), ("T", (B, S)), ("sem", (B, n_sem)))}
    L = _lib.lib()

    def run(noise, rng):
        o = {n: torch.full(s, float("nan"), device=DEV)
             for n, s in (("rgb", (B, 3)), ("depth", (B,)), ("w", (B, S)), ("T", (B, S)), ("sem", (B, n_sem)))}
        full = not weights_only
        _lib.check(L.spnerf_composite_forward(B, S, _lib.ptr(z), _lib.ptr(raw_d), NO, _lib.ptr(noise), 1.0, 8, n_sem, flags,
                                              _lib.ptr(o["rgb"] if full else None), _lib.ptr(o["depth"]), _lib.ptr(o["w"]),
                                              _lib.ptr(o["T"]), _lib.ptr(o["sem"] if full else None), _lib.rng_ref(rng),
                                              _lib.stream_of(z)), "composite_forward")
        d_out = torch.full((B * S, NO), float("nan"), device=DEV)
        _lib.check(L.spnerf_composite_backward(B, S, _lib.ptr(z), _lib.ptr(raw_d), NO, _lib.ptr(noise), 1.0, 8, n_sem, flags,
                                               _lib.ptr(grads["rgb"] if full else None), _lib.ptr(grads["depth"]),
                                               _lib.ptr(grads["w"]), _lib.ptr(grads["T"]),
                                               _lib.ptr(grads["sem"] if full else None), _lib.ptr(d_out),
                                               _lib.rng_ref(rng), _lib.stream_of(z)), "composite_backward")
        if weights_only:
            del o["rgb"], o["sem"]
        o["d_out"] = d_out
        return o

    noise = k.fill(1, B, S)
    got, want = run(None, k.rng), run(noise, None)
    quiet = run(torch.zeros_like(noise), None)
    assert not torch.equal(quiet["w"], want["w"])            # the noise matters at these σ
    for n in want:
        assert torch.isfinite(want[n]).all(), n
        assert torch.equal(got[n], want[n]), n


# ---- a whole render under PhiloxRandom = the render replaying the reference's draw list --------

def _render(name, src, reuse):
    data = gu.load(name)
    meta = data["meta"]
    dims, args = gu.dims_of(meta), gu.args_of(meta)
    args.noise_std = 1.0
    models = {"coarse": make_model(dims, meta["seed"])}
    params = dict(models["coarse"].named_parameters())
    if args.n_importance > 0:
        models["fine"] = make_model(dims, meta["seed"] + 100)
        params.update({"fine." + n: p for n, p in models["fine"].named_parameters()})
    sem = torch.tensor(data["in_semantics"], device=DEV) if "in_semantics" in data else None
    kw = dict(valid_depth=torch.tensor(data["in_valid_depth"], device=DEV),
              target_depths=torch.tensor(data["in_target_depths"], device=DEV),
              target_std=torch.tensor(data["in_target_std"], device=DEV))
    old = rendering.REUSE_PASS1
    rendering.REUSE_PASS1 = reuse
    try:
        with random_source(src):
            res = spnerf_amd.render_rays(models, args, torch.tensor(data["rays"], device=DEV), None, semantics=sem,
                                         mode="train", **kw)
    finally:
        rendering.REUSE_PASS1 = old
    shapes = {k: tuple(v.shape) for k, v in res.items() if torch.is_tensor(v) and v.requires_grad}
    R = gu.projection_weights(shapes)
    sum((res[k] * torch.tensor(R[k], device=DEV)).sum() for k in sorted(R)).backward()
    outs = {k: v.detach().cpu() for k, v in res.items() if torch.is_tensor(v)}
    grads = {n: p.grad.detach().cpu().clone() for n, p in params.items() if p.grad is not None}
    return outs, grads


@pytest.mark.parametrize("name,reuse", [("c3_w64", True), ("c3_w64", False), ("fine_sc_guided_w64", True)])
def test_philox_render_equals_replayed_reference_draws(name, reuse):
    seed, ray0, step = 11, 1000, 5
    src = PhiloxRandom(seed=seed, ray_offset=ray0)
    src.reset_step(step - 1)
    outs, grads = _render(name, src, reuse)
    assert src.sync_host_step() == step

    data = gu.load(name)
    args = gu.args_of(data["meta"])
    B, S = data["rays"].shape[0], args.n_samples
    filler = PhiloxRandom(seed=seed, ray_offset=ray0)      # the same key, for the normals
    filler.reset_step(step - 1)
    filler.begin_render(DEV)
    draws = pr.render_draws(seed, step, ray0, B, S, guided=args.guidedsample, valid=data["in_valid_depth"],
                            solar=args.sc_lambda > 0, n_importance=args.n_importance,
                            normal_fn=lambda slot, n: filler.fill("randn", B, n, slot).cpu().numpy())
    replay = ReplayRandom(draws)
    outs_r, grads_r = _render(name, replay, reuse)
    assert replay.used == len(draws), "the render took fewer draw streams than the slot table lists"
    assert sorted(outs) == sorted(outs_r) and sorted(grads) == sorted(grads_r) and grads
    for k in outs_r:
        assert torch.isfinite(outs_r[k]).all(), k
        assert torch.equal(outs[k], outs_r[k]), k
    for n in grads_r:
        assert torch.equal(grads[n], grads_r[n]), n
