"""bf16 MLP kernels vs the float64 model of their own roundings (oracle/bf16_emu.py) — needs an MI355X.

tests/test_gpu_bf16.py holds the bf16 path to the fp32 reference fixtures at bounds as wide as the
bf16 noise itself (OUT_TOL_KEY, GRAD_TOL = 8e-2).  Here the comparison partner makes the SAME bf16
roundings in float64, so what is left is fp32 accumulation order, the hardware sine / exponential
and the bf16 roundings those flip.  Checked per output key and per parameter tensor, for EVERY
parameter tensor (the sigma / sun / beta output biases included), on shapes picked for their edges
(bf16_emu_cases.py): one point, one short of / exactly / one over the 64- and 128-point tiles, a
ragged last tile, PE off, every width the kernels take another path for, every class label and
-100, the beta head with its time rows, the solar pass's two-segment weight gradients, a guided
pass teacher-forced with the kernel's own depths - at the library defaults and with fused_trunk = 0
(both ends of the bitwise chain of test_gpu_trunk.py).

Bounds: bf16_emu_cases.BOUNDS[key] = (worst distance measured on the MI355X, bound = 3x it), side by
side there.  Measured: one point agrees to 8e-8 on every column (no rounding site is missing); from
63 points on the distance is set by rounding flips that cascade through the eight rounded layers:
per-point columns 1-6e-4 (logits 2e-3), composited keys 1-3e-5, rgb 2e-4, gradients 2-7e-3 per
tensor against 1-5e-2 for the fp32 fixtures.  The two conditions on the bounds are checked on the CPU
(tests/test_bf16_emu_ref.py::test_bounds_against_mutations_and_loose_bounds): seven of the eight
mutations move some key by at least twice its bound (not l0_hi_only: NOT_DETECTABLE there); depth,
weights, transparency and sigma are under 1/8 of their loose bound, the others reach 1/2 to 1/6
(bf16_emu_cases.OVER_EIGHTH) and are reported as measured, not relaxed.
"""
import numpy as np
import pytest
import torch

import bf16_emu_cases as cases
import golden_util as gu
import spnerf_amd
from spnerf_amd import ReplayRandom, _lib, random_source
from test_gpu_parity import DEV, make_model

pytestmark = pytest.mark.gpu


def bound(key: str) -> float:
    return cases.BOUNDS[key][1]


def _check(name, errs):
    """errs: {label: (bound key, error)}; prints every figure before it asserts."""
    worst = {}
    for label, (bk, e) in errs.items():
        worst[bk] = max(worst.get(bk, 0.0), e)
    print("MEASURED", name, {k: f"{v:.3e}" for k, v in sorted(worst.items())})
    bad = {label: (e, bound(bk)) for label, (bk, e) in errs.items() if not e <= bound(bk)}
    assert not bad, (name, bad)


@pytest.mark.parametrize("cid,dims,P", cases.POINT_CASES, ids=[c[0] for c in cases.POINT_CASES])
def test_point_network_matches_emulation(cid, dims, P):
    xyz, sun, lab, t = cases.point_inputs(dims, P)
    m = make_model(dims, cases.SEED_W, "bf16")
    out = m(torch.tensor(xyz, device=DEV), input_sun_dir=torch.tensor(sun, device=DEV),
            input_t=torch.tensor(t, device=DEV) if dims.beta else None,
            input_s=torch.tensor(lab, device=DEV) if dims.sem else None).detach().cpu().numpy()
    ref = cases.point_emulation(dims, P)
    assert out.shape == ref.shape and np.isfinite(out).all()
    cols = {"albedo": slice(0, 3), "sigma": slice(3, 4), "sun": slice(4, 5), "sky": slice(5, 8)}
    c = 8
    if dims.beta:
        cols["beta"] = slice(c, c + 1)
        c += 1
    if dims.sem:
        cols["point_logits"] = slice(c, None)
    _check(cid, {k: (k, gu.rel_err(out[:, s], ref[:, s])) for k, s in cols.items()})


def _kernel_train(name, options):
    c = cases.train_inputs(name)
    dims = c["dims"]
    saved = {k: _lib.get_option(k) for k in options}
    for k, v in options.items():
        _lib.set_option(k, v)
    try:
        model = make_model(dims, cases.SEED_W, "bf16")
        models, params = {"coarse": model}, dict(model.named_parameters())
        ts = None
        if dims.beta:
            emb = torch.nn.Embedding(*c["t_weight"].shape).to(DEV)
            with torch.no_grad():
                emb.weight.copy_(torch.tensor(c["t_weight"]))
            models["t"], params["t.weight"] = emb, emb.weight
            ts = torch.tensor(c["ts"], device=DEV)
        kw = {}
        if c["guided"]:
            kw = dict(valid_depth=torch.tensor(c["valid"], device=DEV), target_depths=torch.tensor(c["target_depths"], device=DEV),
                      target_std=torch.tensor(c["target_std"], device=DEV))
        sem = torch.tensor(c["sem"], device=DEV) if dims.sem else None
        with random_source(ReplayRandom(c["draws"])) as src:
            res = spnerf_amd.render_rays(models, c["args"], torch.tensor(c["rays"], device=DEV), ts, semantics=sem,
                                         mode="train", **kw)
        assert src.used == len(src.draws), "random draws consumed differ from the case's list"
        keys = sorted(k for k, v in res.items() if v.requires_grad)
        cases.projection_loss(res, keys, DEV).backward()
        torch.cuda.synchronize()
        return ({k: v.detach().cpu() for k, v in res.items()},
                {n: (p.grad.detach().cpu().numpy() if p.grad is not None else np.zeros(tuple(p.shape), np.float32))
                 for n, p in params.items()}, keys)
    finally:
        for k, v in saved.items():
            _lib.set_option(k, v)


_EMU = {}   # case -> (z_vals the emulation ran at, outputs, gradients): computed once, shared by the option variants


def _emulation(name, z_vals, keys):
    if name not in _EMU:
        _EMU[name] = (z_vals.clone(),) + cases.emulate_train(name, z_vals, keys=keys)
    z0, outs, grads = _EMU[name]
    assert torch.equal(z0, z_vals), "the option variants of a case must sample the same depths"
    return outs, grads


TRAIN_RUNS = [(n, {}) for n in cases.TRAIN_CASES] + [(n, {"fused_trunk": 0}) for n in ("w512_sem_33x32", "w512_sem_257x64_sc")]


@pytest.mark.parametrize("name,options", TRAIN_RUNS, ids=[n + "".join(f"-{k}{v}" for k, v in o.items()) for n, o in TRAIN_RUNS])
def test_training_render_matches_emulation(name, options):
    res, grads, keys = _kernel_train(name, options)
    c = cases.train_inputs(name)
    z = res["z_vals_coarse"]
    if not c["guided"]:   # stratified depths do not depend on the network
        assert gu.rel_err(z.numpy(), cases.stratified_z(c).numpy()) < 1e-6
    eo, eg = _emulation(name, z, keys)   # guided: teacher-forced with the kernel's own depths
    assert set(keys) <= set(eo), (keys, sorted(eo))
    errs = {}
    for k, ref in eo.items():
        got = res[k].numpy()
        assert got.shape == ref.shape and np.isfinite(got).all(), k
        errs[k] = (cases.out_stem(k), gu.rel_err(got, ref))
    assert sorted(grads) == sorted(eg)
    for n, ref in eg.items():   # EVERY parameter tensor, the scalar output biases included
        if np.any(ref):
            errs["grad " + n] = (cases.param_class(n), gu.rel_err(grads[n], ref))
        else:
            assert not np.any(grads[n]), n
    tag = name + "".join(f"-{k}{v}" for k, v in options.items())
    print("PER_TENSOR", tag, {k: f"{e:.2e}" for k, (_, e) in errs.items()})
    _check(tag, errs)
