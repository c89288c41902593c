"""Float64 model of the per-point network AS THE bf16 KERNELS ROUND IT — TEST INFRASTRUCTURE ONLY.

``ref_cpu.field`` is the network in exact arithmetic; the bf16 MLP (``SPNeRF(precision="bf16")``)
differs from it by its roundings to bf16.  This module makes the same roundings in float64, so
that what is left between it and the kernels is fp32 accumulation order, the hardware sine /
exponential and the few bf16 roundings those flip.  Every rounding site is a switch of
``EmuSites``; with every switch off ``emu_field`` IS ``ref_cpu.field`` in float64
(``tests/test_bf16_emu_ref.py``).  The sites, and where the kernels make them:

* ``w_bf16``    GEMM weights packed as bf16 (``csrc/pack.hip`` pack_params, pieces with bf = 1 / 2
                / 5 / 7): ``fc_net.2i`` for i >= 1 (the skip layer's H and PE columns),
                ``feats_from_xyz``, ``logit_from_label.0``, the first ``width`` columns of
                ``sun_v_net.0`` and ``beta_from_xyz.0``, ``rgb_from_xyzdir.0``, ``sun_v_net.2 / .4``.
                fp32 stay: every bias, the semantic / sun-direction / time columns (per-ray rows,
                ``k_ray_fwd``), the embedding, the narrow heads (σ, rgb.2, sun_v.6, β.2, logits.2)
                and the sky MLP;
* ``l0_split``  ``fc_net.0`` as (x_hi + x_lo)·(w_hi + w_lo) with hi = bf16(v), lo = bf16(v − hi)
                (pack.hip bf = 3 / 4: planes [hi | hi | lo | lo] against the input's [hi | lo | hi | lo],
                i.e. all four products of the K = 4·K0p GEMM);
* ``act_bf16``  every activation stored as bf16 after bias → per-ray row → sin(w0·v)
                (``gemm_bf16.hip`` / ``trunk_bf16.hip`` epilogues): the trunk's H_i, the semantic hidden
                layer, Q = [sun_v.0 | rgb.0 | β.0], sun_v.2 / .4's outputs — and the linear ``feat``;
* ``pe_bf16``   the skip layer and fc_net.0's weight gradient read the bf16 copy of the PE rows
                (X0b; layer 0's forward reads the hi/lo planes);
* ``d_bf16``    backward: the saved derivative D = bf16(w0·cos(w0·v)) multiplies dH
                (``k_trunk_bwd_bf16``, ``heads_dx_bf16.hip``, the ×D GEMM epilogues of ``mlp_backward.hip``);
* ``dz_bf16``   backward: dZ = dH ⊙ D is stored as bf16, and so is d feat.  Every weight / bias /
                per-ray-row gradient downstream is a sum over these rounded dZ (fp32 sums in the
                kernels, float64 here).
The narrow heads read bf16-rounded inputs with fp32 weights and the 1.002·x − 0.001 albedo map,
softplus and the sky MLP are fp32 in the kernels: float64 here, no switch (the fused heads' hi/lo
rows for σ / rgb.2 / sun_v.6 carry 2^-17 per weight: under 1e-5 of any output).

``mut`` names one deliberate kernel bug (``MUTATIONS``) for the discrimination table of
``tests/test_bf16_emu_ref.py``.
"""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Dict, Optional

import torch
import torch.nn.functional as F

from . import ref_cpu
from .weights import ModelDims

Tensor = torch.Tensor
Params = Dict[str, Tensor]


@dataclass(frozen=True)
class EmuSites:
    w_bf16: bool = True
    l0_split: bool = True
    act_bf16: bool = True
    pe_bf16: bool = True
    d_bf16: bool = True
    dz_bf16: bool = True

    @staticmethod
    def off() -> "EmuSites":
        return EmuSites(False, False, False, False, False, False)

    def without(self, name: str) -> "EmuSites":
        return replace(self, **{name: False})


SITES = ("w_bf16", "l0_split", "act_bf16", "pe_bf16", "d_bf16", "dz_bf16")
FORWARD_SITES = ("w_bf16", "l0_split", "act_bf16", "pe_bf16")

# kernel bugs we could plausibly ship; TILE = the trunk's 64-point tile
MUTATIONS = ("drop_k32_last_tile", "skip_pe_zero_tile", "l0_hi_only", "pad_is_class0", "bias_tail16",
             "swap_rows_last_tile", "wgrad_split_missing", "sigma_bias_last_tile")
TILE = 64
MUT_LAYER = 2       # the trunk layer the single-layer mutations hit
WGRAD_SPLIT = 256   # points per split of the weight-gradient GEMMs


def rbf(x: Tensor) -> Tensor:
    """Round to nearest even to bf16, through fp32 (as the kernels' fp32 -> bf16 conversions)."""
    return x.float().bfloat16().double()


class _RoundSTE(torch.autograd.Function):
    """A parameter as the pack rounds it; the gradient goes to the fp32 master unchanged."""

    @staticmethod
    def forward(ctx, w):
        return rbf(w)

    @staticmethod
    def backward(ctx, g):
        return g


class _SplitSTE(torch.autograd.Function):
    """hi + lo bf16 planes of a parameter (hi_only: the hi plane alone)."""

    @staticmethod
    def forward(ctx, w, hi_only):
        hi = rbf(w)
        return hi if hi_only else hi + rbf(w - hi)

    @staticmethod
    def backward(ctx, g):
        return g, None


class _Act(torch.autograd.Function):
    """y = sin(w0·z) stored as bf16; backward dZ = bf16(dY ⊙ D) with the saved D = bf16(w0·cos(w0·z))."""

    @staticmethod
    def forward(ctx, z, w0, s):
        y = torch.sin(w0 * z)
        dd = w0 * torch.cos(w0 * z)
        ctx.save_for_backward(rbf(dd) if s.d_bf16 else dd)
        ctx.dz = s.dz_bf16
        return rbf(y) if s.act_bf16 else y

    @staticmethod
    def backward(ctx, g):
        (dd,) = ctx.saved_tensors
        dz = g * dd
        return (rbf(dz) if ctx.dz else dz), None, None


class _Store(torch.autograd.Function):
    """A linear GEMM output stored as bf16 (feat); its gradient is stored as bf16 too."""

    @staticmethod
    def forward(ctx, x, s):
        ctx.dz = s.dz_bf16
        return rbf(x) if s.act_bf16 else x

    @staticmethod
    def backward(ctx, g):
        return (rbf(g) if ctx.dz else g), None


class _Lin(torch.autograd.Function):
    """x·wᵀ (+ b).  ``xw``: what the weight gradient reads in x's place (fc_net.0: the bf16 PE rows);
    ``skip_w`` / ``skip_b``: point ranges a mutated weight / bias gradient leaves out of its sum."""

    @staticmethod
    def forward(ctx, x, w, b, xw, skip_w, skip_b):
        ctx.save_for_backward(x if xw is None else xw, w)
        ctx.skips = (skip_w, skip_b)
        ctx.x_grad = x.requires_grad
        z = x @ w.t()
        return z if b is None else z + b

    @staticmethod
    def backward(ctx, g):
        xw, w = ctx.saved_tensors
        skip_w, skip_b = ctx.skips
        gw = gb = g
        if skip_w is not None:
            gw = g.clone()
            gw[skip_w[0]:skip_w[1]] = 0
        if skip_b is not None:
            gb = g.clone()
            gb[skip_b[0]:skip_b[1]] = 0
        return (g @ w if ctx.x_grad else None), gw.t() @ xw, (gb.sum(0) if ctx.needs_input_grad[2] else None), None, None, None


def _lin(x, w, b=None, xw=None, skip_w=None, skip_b=None):
    return _Lin.apply(x, w, b, xw, skip_w, skip_b)


def last_tile(P: int):
    """[begin, end) of the ragged last 64-point tile."""
    return ((P - 1) // TILE) * TILE, P


def emu_field(p: Params, d: ModelDims, xyz: Tensor, sun_d: Tensor, labels: Optional[Tensor] = None,
              t_emb: Optional[Tensor] = None, sites: EmuSites = EmuSites(), mode: str = "full",
              mut: Optional[str] = None) -> Tensor:
    """``ref_cpu.field`` with the bf16 MLP's roundings: float64 (P, 3) points → (P, n_outputs).
    mode "sun": the solar pass (σ and sun only; the other columns are zero)."""
    assert mut is None or mut in MUTATIONS, mut
    s = sites
    P, W, K0 = xyz.shape[0], d.width, d.in_xyz
    t0, t1 = last_tile(P)
    rw = (lambda w: _RoundSTE.apply(w)) if s.w_bf16 else (lambda w: w)
    act = lambda z, w0=1.0: _Act.apply(z, w0, s)
    enc = ref_cpu.posenc(xyz, d.n_freq) if d.mapping else xyz
    emb = None
    if d.sem and labels is not None:
        lab = labels.reshape(-1).long()
        pad = 0 if mut == "pad_is_class0" else d.num_sem_classes
        lab = torch.where(lab == -100, torch.full_like(lab, pad), lab)
        emb = F.embedding(lab, p["semantic_embedding.weight"], padding_idx=d.num_sem_classes)
    pe_b = rbf(enc) if s.pe_bf16 else enc                     # X0b: the bf16 copy of the PE rows
    if mut == "skip_pe_zero_tile":
        pe_b = pe_b.clone()
        m0 = TILE if P > TILE else 0                           # the second tile where there is one
        pe_b[m0:m0 + TILE] = 0

    def bias_of(i):
        b = p[f"fc_net.{2 * i}.bias"]
        if mut == "bias_tail16" and i == MUT_LAYER:
            b = torch.cat([b[:-16], torch.zeros_like(b[-16:])])
        return b

    # fc_net.0: hi/lo planes of the PE rows against hi/lo planes of the weights; semantic columns as
    # fp32 rows; the weight gradient reads the bf16 PE rows
    w0 = p["fc_net.0.weight"]
    if s.l0_split:
        hi = rbf(enc)
        x0 = hi if mut == "l0_hi_only" else hi + rbf(enc - hi)
        wx = _SplitSTE.apply(w0[:, :K0], mut == "l0_hi_only")
    else:
        x0, wx = enc, w0[:, :K0]
    z = _lin(x0, wx, bias_of(0), xw=pe_b if s.pe_bf16 else None)
    if emb is not None:
        z = z + emb @ w0[:, K0:].t()
    h = act(z, 30.0)
    for i in range(1, d.layers):
        wi = p[f"fc_net.{2 * i}.weight"]
        hin = h
        if mut == "drop_k32_last_tile" and i == MUT_LAYER:
            hin = h.clone()
            hin[t0:t1, W - 32:] = 0
        skip_w = None
        if mut == "wgrad_split_missing" and i == MUT_LAYER:
            skip_w = (0, min(WGRAD_SPLIT, P))
        z = _lin(hin, rw(wi[:, :W]), bias_of(i), skip_w=skip_w)
        if i in d.skips:
            z = z + pe_b @ rw(wi[:, W:W + K0]).t()
            if emb is not None:
                z = z + emb @ wi[:, W + K0:].t()
        h = act(z)
    NO = d.n_outputs
    sig = F.softplus(_lin(h, p["sigma_from_xyz.0.weight"], p["sigma_from_xyz.0.bias"],
                          skip_b=(t0, t1) if mut == "sigma_bias_last_tile" else None))
    feat = _Store.apply(_lin(h, rw(p["feats_from_xyz.weight"]), p["feats_from_xyz.bias"]), s)
    ws1 = p["sun_v_net.0.weight"]
    sv = act(_lin(feat, rw(ws1[:, :W]), p["sun_v_net.0.bias"]) + sun_d @ ws1[:, W:].t())
    for j in (1, 2):
        sv = act(_lin(sv, rw(p[f"sun_v_net.{2 * j}.weight"]), p[f"sun_v_net.{2 * j}.bias"]))
    sun = torch.sigmoid(_lin(sv, p["sun_v_net.6.weight"], p["sun_v_net.6.bias"]))
    if mode == "sun":
        z3, z4 = torch.zeros(P, 3, dtype=xyz.dtype), torch.zeros(P, NO - 5, dtype=xyz.dtype)
        return torch.cat([z3, sig, sun, z4], 1)
    r1 = act(_lin(feat, rw(p["rgb_from_xyzdir.0.weight"]), p["rgb_from_xyzdir.0.bias"]))
    rgb = torch.sigmoid(_lin(r1, p["rgb_from_xyzdir.2.weight"], p["rgb_from_xyzdir.2.bias"])) * 1.002 - 0.001
    sky = torch.sigmoid(ref_cpu._lin(p, "sky_color.2", torch.relu(ref_cpu._lin(p, "sky_color.0", sun_d))))
    cols = [rgb, sig, sun, sky]
    if d.beta:
        wb = p["beta_from_xyz.0.weight"]
        bh = act(_lin(feat, rw(wb[:, :W]), p["beta_from_xyz.0.bias"]) + t_emb @ wb[:, W:].t())
        cols.append(F.softplus(_lin(bh, p["beta_from_xyz.2.weight"], p["beta_from_xyz.2.bias"])))
    if d.sem:
        mh = act(_lin(h, rw(p["logit_from_label.0.weight"]), p["logit_from_label.0.bias"]))
        cols.append(_lin(mh, p["logit_from_label.2.weight"], p["logit_from_label.2.bias"]))
    out = torch.cat(cols, 1)
    if mut == "swap_rows_last_tile" and P >= 2:
        idx = torch.arange(P)
        idx[P - 2], idx[P - 1] = P - 1, P - 2
        out = out[idx]
    return out


def points_f32(rays: Tensor, z: Tensor, dir_col: int) -> Tensor:
    """o + dir·z as the kernels form it (``trunk.h`` pe_value): two rounded fp32 operations."""
    o, dv = rays[:, None, 0:3].float(), rays[:, None, dir_col:dir_col + 3].float()
    return (o + dv * z.float()[:, :, None]).reshape(-1, 3)


def emu_render(p: Params, d: ModelDims, rays: Tensor, z_vals: Tensor, noise: Optional[Tensor], noise_std: float,
               labels: Optional[Tensor] = None, t_emb: Optional[Tensor] = None, sites: EmuSites = EmuSites(),
               solar: bool = False, mut: Optional[str] = None) -> Dict[str, Tensor]:
    """One inference() pass (``ref_cpu.inference``) at given depths and σ-noise: the emulated field
    at the fp32 points of ``rays`` (B, 11) and ``z_vals`` (B, S), then ``ref_cpu.composite`` in
    float64.  ``solar``: the solar-correction pass (points along the sun direction, σ and sun only)."""
    B, S = z_vals.shape
    rep = lambda v: None if v is None else torch.repeat_interleave(v, S, dim=0)
    xyz = points_f32(rays, z_vals, 8 if solar else 3).double()
    sun_d = rays[:, 8:11].double()
    out = emu_field(p, d, xyz, rep(sun_d), rep(labels), rep(None if t_emb is None else t_emb.double()), sites,
                    "sun" if solar else "full", mut).view(B, S, d.n_outputs)
    zd = z_vals.double()
    rgb, depth, w, trans = ref_cpu.composite(out, zd, None if noise is None else noise.double(), noise_std)
    res = {"depth": depth, "weights": w, "transparency": trans, "sun": out[..., 4:5]}
    if solar:
        return res
    res.update({"rgb": rgb, "albedo": out[..., :3], "sky": out[..., 5:8]})
    col = 8
    if d.beta:
        res["beta"] = out[..., col:col + 1]
        col += 1
    if d.sem:
        res["sem_logits"] = torch.mean(out[..., col:], dim=1)
    return res


def emu_render_rays(p: Params, d: ModelDims, rays: Tensor, z_vals: Tensor, noise, noise_std: float, labels=None,
                    t_emb=None, sites: EmuSites = EmuSites(), noise_sc=None, mut: Optional[str] = None) -> Dict[str, Tensor]:
    """The coarse keys of ``render_rays`` at given depths: the main pass, and with ``noise_sc`` given
    (the solar pass's σ-noise; sc_lambda > 0) the solar pass's weights_sc / transparency_sc / sun_sc."""
    res = emu_render(p, d, rays, z_vals, noise, noise_std, labels, t_emb, sites, False, mut)
    if noise_sc is not None:
        sc = emu_render(p, d, rays, z_vals, noise_sc, noise_std, labels, t_emb, sites, True, mut)
        res["weights_sc"], res["transparency_sc"], res["sun_sc"] = sc["weights"], sc["transparency"], sc["sun"]
    return {f"{k}_coarse": v for k, v in res.items()}


def params64(weights: dict, requires_grad: bool = True) -> Params:
    return {k: torch.tensor(v, dtype=torch.float64).requires_grad_(requires_grad) for k, v in weights.items()}
