"""Training losses over the render dictionary — drop-in for modules/metrics.py of the reference.

Same classes, constructor arguments, dictionary keys and reductions as metrics.py:
``uncertainty_aware_loss`` :10-14, ``solar_correction`` :17-24, ``SNerfLoss`` :27-45,
``SatNerfLoss`` :48-65, ``DepthLoss`` :68-159 (subset MSE, subset GNLL, use-all-depth),
``SemanticLoss`` :162-183, ``load_loss`` :186-194, ``mse`` / ``psnr`` :197-207, each with its
``*_fine`` terms when the render carries fine keys.  These are plain torch on (B, ·) tensors and
pinned to the reference's own values and gradients (tests/golden/losses.npz,
tests/test_losses.py).

One deliberate difference, not in the values: the reference selects the depth-loss rays with
boolean indexing, a device→host count per step; here the same sums run under a 0/1 mask, so a
step has no host synchronisation and can be captured in a HIP graph.

For the training step's own combination (SNerfLoss with the solar terms + subset MSE depth
loss + semantic cross-entropy) ``FusedRenderLoss`` computes the loss value and every upstream
gradient in ONE kernel (``spnerf_render_loss``, csrc/loss.hip) instead of ~60 small ATen launches.
"""
from __future__ import annotations

import ctypes

import torch


def uncertainty_aware_loss(loss_dict, inputs, gt_rgb, typ, beta_min=0.05):
    """metrics.py:10-14 (β of the COARSE pass weights either pass's colour, as there)."""
    beta = torch.sum(inputs[f"weights_{typ}"].unsqueeze(-1) * inputs["beta_coarse"], -2) + beta_min
    loss_dict[f"{typ}_color"] = ((inputs[f"rgb_{typ}"] - gt_rgb) ** 2 / (2 * beta ** 2)).mean()
    loss_dict[f"{typ}_logbeta"] = (3 + torch.log(beta).mean()) / 2
    return loss_dict


def solar_correction(loss_dict, inputs, typ, lambda_sc=0.05):
    """metrics.py:17-24: Shadow-NeRF terms 2 and 3 (transparency / weights of the solar pass
    detached: only sun_sc receives a gradient)."""
    sun_sc = inputs[f"sun_sc_{typ}"].squeeze()
    term2 = torch.sum(torch.square(inputs[f"transparency_sc_{typ}"].detach() - sun_sc), -1)
    term3 = 1 - torch.sum(inputs[f"weights_sc_{typ}"].detach() * sun_sc, -1)
    loss_dict[f"{typ}_sc_term2"] = lambda_sc / 3.0 * torch.mean(term2)
    loss_dict[f"{typ}_sc_term3"] = lambda_sc / 3.0 * torch.mean(term3)
    return loss_dict


class SNerfLoss(torch.nn.Module):
    """metrics.py:27-45."""

    def __init__(self, lambda_sc=0.05):
        super().__init__()
        self.lambda_sc = lambda_sc
        self.loss = torch.nn.MSELoss(reduction="mean")

    def forward(self, inputs, targets):
        loss_dict = {}
        for typ in ("coarse", "fine"):
            if typ == "fine" and "rgb_fine" not in inputs:
                break
            loss_dict[f"{typ}_color"] = self.loss(inputs[f"rgb_{typ}"], targets)
            if self.lambda_sc > 0:
                loss_dict = solar_correction(loss_dict, inputs, typ, self.lambda_sc)
        return sum(loss_dict.values()), loss_dict


class SatNerfLoss(torch.nn.Module):
    """metrics.py:48-65: colour weighted by the rendered uncertainty β, plus log β."""

    def __init__(self, lambda_sc=0.0):
        super().__init__()
        self.lambda_sc = lambda_sc

    def forward(self, inputs, targets):
        loss_dict = {}
        for typ in ("coarse", "fine"):
            if typ == "fine" and "rgb_fine" not in inputs:
                break
            loss_dict = uncertainty_aware_loss(loss_dict, inputs, targets, typ)
            if self.lambda_sc > 0:
                loss_dict = solar_correction(loss_dict, inputs, typ, self.lambda_sc)
        return sum(loss_dict.values()), loss_dict


def _gaussian_nll(inp, target, var, eps=1e-6):
    """Elementwise torch.nn.GaussianNLLLoss (full=False): the variance is clamped to eps with
    the clamp invisible to autograd, as torch does."""
    var = var + (var.clamp(min=eps) - var).detach()
    return 0.5 * (torch.log(var) + (inp - target) ** 2 / var)


class DepthLoss(torch.nn.Module):
    """metrics.py:68-159.  ``usealldepth`` (the reference default): λ/3 · mean(w · (d − t)²) over
    all rays.  Otherwise the subset form: rays with a depth prior (valid) whose prediction lies
    outside the expected distribution (|d − t| > σ_t or σ_pred > σ_t, :78-80), each term scaled by
    n_applied / B (:125-127) before the mean over the applied rays — i.e. λ/3 · Σ_applied term / B;
    term = w · (d − t)² (MSE) or the Gaussian NLL with variance σ_pred (GNLL, :129-130), where
    σ_pred = sqrt(Σ weights · (z − d)²) (:102) carries a gradient in the GNLL form only."""

    def __init__(self, lambda_ds=1.0, GNLL=False, usealldepth=True, margin=0, stdscale=1):
        super().__init__()
        self.lambda_ds = lambda_ds / 3.0
        self.GNLL = GNLL
        self.usealldepth = usealldepth
        self.margin = margin
        self.stdscale = stdscale

    @staticmethod
    def is_not_in_expected_distribution(pred_depth, pred_std, target_depth, target_std):
        depth_diff = (pred_depth - target_depth).abs()
        return torch.logical_or(depth_diff > target_std, pred_std > target_std)

    def subset_term(self, inputs, typ, target_depth, target_weight, target_valid_depth, target_std):
        z, pd, pw = inputs[f"z_vals_{typ}"], inputs[f"depth_{typ}"], inputs[f"weights_{typ}"]
        if target_valid_depth is None:
            target_valid_depth = torch.ones(pd.shape[0], device=pd.device)
        B = float(target_valid_depth.shape[0])
        var = ((z - pd.unsqueeze(-1)).pow(2) * pw).sum(-1)
        with torch.no_grad():
            apply = (target_valid_depth > 0) & self.is_not_in_expected_distribution(pd, var.sqrt(), target_depth, target_std)
            m = apply.to(pd.dtype)
        if self.GNLL:
            # σ_pred only on the applied rays (metrics.py:90-102 computes it for those alone): a
            # ray left out with zero spread must not put sqrt'(0) = inf · 0 = NaN into the gradient
            pstd = torch.where(apply, var, torch.ones_like(var)).sqrt()
            term = _gaussian_nll(pd, target_depth, torch.where(apply, pstd, torch.ones_like(pstd)))
        else:
            term = target_weight * (pd - target_depth) ** 2
        return self.lambda_ds * torch.sum(m * term) / B

    def forward(self, inputs, targets, weights=1.0, target_valid_depth=None, target_std=None):
        loss_dict = {}
        for typ in ("coarse", "fine"):
            if typ == "fine" and "depth_fine" not in inputs:
                break
            if self.usealldepth:
                loss_dict[f"{typ}_ds"] = self.lambda_ds * torch.mean(weights * (inputs[f"depth_{typ}"] - targets) ** 2)
            else:
                loss_dict[f"{typ}_ds"] = self.subset_term(inputs, typ, targets, weights, target_valid_depth, target_std)
        return sum(loss_dict.values()), loss_dict


class SemanticLoss(torch.nn.Module):
    """metrics.py:162-183: cross-entropy of the ray's mean semantic logits, ignore_index −100."""

    def __init__(self, lambda_ss=1.0):
        super().__init__()
        self.lambda_ss = lambda_ss
        self.cross_entropy_loss = torch.nn.CrossEntropyLoss(ignore_index=-100)

    def forward(self, inputs, targets):
        loss_dict = {"coarse_ss": self.cross_entropy_loss(inputs["sem_logits_coarse"], targets)}
        if "sem_logits_fine" in inputs:
            loss_dict["fine_ss"] = self.cross_entropy_loss(inputs["sem_logits_fine"], targets)
        for k in loss_dict:
            loss_dict[k] = self.lambda_ss * loss_dict[k]
        return sum(loss_dict.values()), loss_dict


def load_loss(args):
    """metrics.py:186-194."""
    if args.model == "sp-nerf":
        return SatNerfLoss(lambda_sc=args.sc_lambda) if args.beta else SNerfLoss(lambda_sc=args.sc_lambda)
    raise ValueError(f"model {args.model} is not valid")


def mse(image_pred, image_gt, valid_mask=None, reduction="mean"):
    value = (image_pred - image_gt) ** 2
    if valid_mask is not None:
        value = value[valid_mask]
    if reduction == "mean":
        return torch.mean(value)
    return value


def psnr(image_pred, image_gt, valid_mask=None, reduction="mean"):
    return -10 * torch.log10(mse(image_pred, image_gt, valid_mask, reduction))


from .image import ssim  # noqa: E402,F401  (metrics.py:210-215, evaluated in fp64 by csrc/ssim.hip)


# ------------------------------------------------------------------------------------------
# fused training loss (csrc/loss.hip)
# ------------------------------------------------------------------------------------------

class _RenderLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rgb, sun_sc, depth, logits, cfg):
        from . import _lib
        L = _lib.lib()
        B, S, C = cfg["B"], cfg["S"], cfg["C"]
        dev = rgb.device
        ws = torch.empty(max(1, L.spnerf_render_loss_workspace_bytes(B) // 4), dtype=torch.float32, device=dev)
        out = torch.empty(7, dtype=torch.float32, device=dev)
        p = _lib.ptr
        _lib.check(L.spnerf_render_loss_forward(
            B, S, C, p(rgb), p(cfg["target"]), cfg["lambda_sc"], p(sun_sc), cfg["ld_sun"], p(cfg["T_sc"]), p(cfg["w_sc"]),
            cfg["lambda_ds"], p(depth), p(cfg["z"]), p(cfg["w"]), p(cfg["td"]), p(cfg["tw"]), cfg["ld_td"], p(cfg["valid"]),
            p(cfg["tstd"]), cfg["lambda_ss"], p(logits), p(cfg["labels"]), p(cfg["labels_global"]), cfg["n_global"],
            cfg["world"], p(ws), p(out), _lib.stream_of(rgb)), "render_loss_forward")
        ctx.cfg = cfg
        ctx.save_for_backward(rgb, sun_sc, depth, logits, out)
        terms = out[1:6]
        ctx.mark_non_differentiable(terms)
        # the terms take no gradient: not materialised as zeros (one fill launch per step)
        ctx.set_materialize_grads(False)
        return out[0], terms

    @staticmethod
    def backward(ctx, g_loss, g_terms):
        from . import _lib
        rgb, sun_sc, depth, logits, out = ctx.saved_tensors
        if g_loss is None:
            return None, None, None, None, None
        cfg = ctx.cfg
        B, S, C = cfg["B"], cfg["S"], cfg["C"]
        g = g_loss.contiguous().reshape(1)
        d_rgb = torch.empty_like(rgb)
        d_sun = torch.empty(B, S, 1, dtype=torch.float32, device=rgb.device) if cfg["lambda_sc"] > 0 else None
        d_depth = torch.empty_like(depth) if cfg["lambda_ds"] > 0 else None
        d_logits = torch.empty_like(logits) if cfg["lambda_ss"] is not None and logits.numel() else None
        p = _lib.ptr
        _lib.check(_lib.lib().spnerf_render_loss_backward(
            B, S, C, p(rgb), p(cfg["target"]), cfg["lambda_sc"], p(sun_sc), cfg["ld_sun"], p(cfg["T_sc"]), p(cfg["w_sc"]),
            cfg["lambda_ds"], p(depth), p(cfg["z"]), p(cfg["w"]), p(cfg["td"]), p(cfg["tw"]), cfg["ld_td"], p(cfg["valid"]),
            p(cfg["tstd"]), cfg["lambda_ss"], p(logits if logits.numel() else None), p(cfg["labels"]), p(out), p(g),
            p(d_rgb), p(d_sun), p(d_depth), p(d_logits), _lib.stream_of(rgb)), "render_loss_backward")
        return d_rgb, d_sun, d_depth, d_logits, None


class FusedRenderLoss(torch.nn.Module):
    """The training step's combined loss in two kernels (csrc/loss.hip): SNerfLoss(lambda_sc)
    + DepthLoss(lambda_ds, usealldepth=False) (MSE form) + SemanticLoss(lambda_ss), as
    main.py:143-174 adds them (coarse keys, no β, no fine model).  Returns (loss, terms) like
    the reference modules, terms = {coarse_color, coarse_sc_term2, coarse_sc_term3, coarse_ds,
    coarse_ss} (0-d device tensors, no gradient).

    ``labels_global`` / ``world`` (data parallelism): the CE mean runs over the valid labels of
    the GLOBAL batch divided by ``world``, so the ranks' losses average to the global one
    (SURVEY §8e pitfall 2); default = this batch, world 1."""

    def __init__(self, lambda_sc=0.05, lambda_ds=0.0, lambda_ss=0.0):
        super().__init__()
        self.lambda_sc, self.lambda_ds, self.lambda_ss = float(lambda_sc), float(lambda_ds), float(lambda_ss)

    def forward(self, inputs, targets, target_depths=None, target_valid_depth=None, target_std=None, semantics=None,
                labels_global=None, world=1):
        from . import _lib
        rgb = inputs["rgb_coarse"]
        _lib.require_device(rgb)
        B = rgb.shape[0]
        dev = rgb.device
        f32 = lambda t: t.contiguous().float()
        cfg = dict(B=B, S=1, C=0, target=f32(targets), lambda_sc=0.0, ld_sun=1, T_sc=None, w_sc=None, lambda_ds=0.0, z=None,
                   w=None, td=None, tw=None, ld_td=2, valid=None, tstd=None, lambda_ss=0.0, labels=None,
                   labels_global=None, n_global=0, world=int(world))
        sun = depth = None
        if self.lambda_sc > 0:
            sun = inputs["sun_sc_coarse"]
            S = sun.shape[1]
            if self.lambda_ds > 0 and inputs["z_vals_coarse"].shape[1] != S:
                raise ValueError(f"FusedRenderLoss: sun_sc has {S} samples per ray, z_vals {inputs['z_vals_coarse'].shape[1]}")
            if sun.stride(1) != sun.stride(0) // S or sun.stride(0) % S:
                sun = sun.contiguous()
            cfg.update(S=S, lambda_sc=self.lambda_sc, ld_sun=sun.stride(1), T_sc=f32(inputs["transparency_sc_coarse"]),
                       w_sc=f32(inputs["weights_sc_coarse"]))
        if self.lambda_ds > 0:
            depth = inputs["depth_coarse"].contiguous()
            z = f32(inputs["z_vals_coarse"])
            td = target_depths.float()
            if td.dim() != 2 or td.stride(1) != 1:
                td = td.contiguous()
            if target_valid_depth is None:   # metrics.py:83-86: every ray has a prior
                target_valid_depth = torch.ones(B, dtype=torch.int64, device=dev)
            cfg.update(S=z.shape[1], lambda_ds=self.lambda_ds, z=z, w=f32(inputs["weights_coarse"].detach()), td=td,
                       tw=td[:, 1:], ld_td=td.stride(0), valid=target_valid_depth.reshape(-1).long().contiguous(),
                       tstd=f32(target_std.reshape(-1)))
        logits = torch.empty(0, device=dev)
        if self.lambda_ss > 0:
            logits = inputs["sem_logits_coarse"].contiguous()
            labels = semantics.reshape(-1).long().contiguous()
            lg = labels if labels_global is None else labels_global.reshape(-1).long().contiguous()
            cfg.update(C=logits.shape[1], lambda_ss=self.lambda_ss, labels=labels, labels_global=lg, n_global=lg.numel())
        if sun is None:
            sun = torch.empty(0, device=dev)
        if depth is None:
            depth = torch.empty(0, device=dev)
        loss, terms = _RenderLoss.apply(rgb.contiguous(), sun, depth, logits, cfg)
        names = ("coarse_color", "coarse_sc_term2", "coarse_sc_term3", "coarse_ds", "coarse_ss")
        return loss, {n: terms[i] for i, n in enumerate(names)}


# ------------------------------------------------------------------------------------------
# fused training loss, every form the trainer combines (csrc/train_loss.hip)
# ------------------------------------------------------------------------------------------

# the differentiable inputs of a pass, in the order _TrainLoss takes them (then beta_coarse)
_PASS_INPUTS = ("rgb", "sun_sc", "depth", "sem_logits", "weights")
_PASS_GRADS = ("d_rgb", "d_sun", "d_depth", "d_logits", "d_weights")


class _TrainLoss(torch.autograd.Function):
    """(cfg, 5 tensors of the coarse pass, 5 of the fine pass, beta_coarse): a slot holds a tensor
    exactly when the configuration sends a gradient there, None otherwise."""

    @staticmethod
    def forward(ctx, cfg, *tensors):
        from . import _lib, _loss_lib
        L = _loss_lib.lib()
        opts, passes = cfg["opts"], cfg["passes"]
        dev = cfg["device"]
        ws = torch.empty(max(1, L.spnerf_train_loss_workspace_bytes(opts.n_rays) // 4), dtype=torch.float32, device=dev)
        out = torch.empty(_loss_lib.RESULT_FLOATS, dtype=torch.float32, device=dev)
        fine = ctypes.byref(passes[1]) if len(passes) > 1 else None
        _lib.check(L.spnerf_train_loss_forward(ctypes.byref(opts), ctypes.byref(passes[0]), fine, _lib.ptr(ws),
                                               _lib.ptr(out), _lib.stream_of(out)), "train_loss_forward")
        ctx.cfg = cfg
        ctx.present = [t is not None for t in tensors]
        ctx.save_for_backward(out, *[t for t in tensors if t is not None])
        terms = out[_loss_lib.PASS_BASE:]
        ctx.mark_non_differentiable(terms)
        # the terms take no gradient: not materialised as zeros (one fill launch per step)
        ctx.set_materialize_grads(False)
        return out[0], terms

    @staticmethod
    def backward(ctx, g_loss, g_terms):
        from . import _lib, _loss_lib
        n = len(ctx.present)
        if g_loss is None:
            return (None,) * (n + 1)
        out, *rest = ctx.saved_tensors
        rest = iter(rest)
        tensors = [next(rest) if p else None for p in ctx.present]
        grads = [None if t is None else torch.empty(t.shape, dtype=torch.float32, device=t.device) for t in tensors]
        cfg = ctx.cfg
        opts, passes = cfg["opts"], cfg["passes"]
        k = len(_PASS_INPUTS)
        for p, ps in enumerate(passes):
            for j, name in enumerate(_PASS_GRADS):
                g = grads[p * k + j]
                setattr(ps, name, None if g is None else g.data_ptr())
        opts.d_beta = None if grads[2 * k] is None else grads[2 * k].data_ptr()
        g = g_loss.contiguous().float().reshape(1)
        fine = ctypes.byref(passes[1]) if len(passes) > 1 else None
        _lib.check(_loss_lib.lib().spnerf_train_loss_backward(ctypes.byref(opts), ctypes.byref(passes[0]), fine,
                                                              _lib.ptr(out), _lib.ptr(g), _lib.stream_of(out)),
                   "train_loss_backward")
        return (None, *grads)


def _column(t, S):
    """A (B, S, 1) or (B, S) column as the kernels read it: element (r, s) at (r·S + s)·ld of the
    pointer.  A strided view of the MLP output (``out.view(B, S, NO)[..., c:c+1]``, as a render
    returns ``sun_sc`` and ``beta``) already is one and is not copied."""
    t = t.float()
    if t.stride(1) != t.stride(0) // S or t.stride(0) % S or t.stride(1) <= 0:
        t = t.contiguous()
    return t, t.stride(1)


class FusedTrainLoss(torch.nn.Module):
    """Every loss form the reference trainer combines (main.py:125-174) in two launches forward
    and one backward (csrc/train_loss.hip, include/spnerf_amd_loss.h), on the coarse keys and, when
    the render carries them, the ``*_fine`` keys:

    * colour: ``SNerfLoss``, or with ``beta=True`` ``SatNerfLoss`` (uncertainty-weighted colour +
      log β; ``beta_coarse`` weights either pass, as in the reference, so the two passes must then
      have equal sample counts);
    * the solar-correction terms when ``lambda_sc > 0``;
    * ``DepthLoss(lambda_ds, GNLL, usealldepth)`` when ``lambda_ds > 0``: subset MSE, subset
      Gaussian NLL (gradients also into ``weights_*``) or use-all-depth; ``target_depths`` is the
      (B, 2) tensor of the dataset (depth, weight);
    * ``SemanticLoss(lambda_ss)`` when ``lambda_ss > 0`` (``labels_global`` / ``world`` as in
      ``FusedRenderLoss``).

    Per call: ``use_beta=False`` selects the plain colour form for a β model (the first two epochs,
    main.py:150-153); ``add_depth=False`` / ``add_sem=False`` still report the term but neither add
    it to the loss nor differentiate it (``ds_drop`` / ``ss_drop``, main.py:163,172).

    Returns ``(loss, terms)``; ``terms`` holds the reference's keys (``{typ}_color``,
    ``{typ}_logbeta``, ``{typ}_sc_term2``, ``{typ}_sc_term3``, ``{typ}_ds``, ``{typ}_ss``) plus
    ``mse_{typ}`` and ``psnr_{typ}`` (train/psnr, main.py:179-181), all 0-d device tensors without
    gradient.  Gradients go to ``rgb_*``, ``sun_sc_*``, ``depth_*``, ``sem_logits_*`` and, for the
    β and GNLL forms, to ``weights_*`` and ``beta_coarse``; no zero gradient is materialised."""

    def __init__(self, lambda_sc=0.05, beta=False, lambda_ds=0.0, GNLL=False, usealldepth=False, lambda_ss=0.0):
        super().__init__()
        self.lambda_sc, self.lambda_ds, self.lambda_ss = float(lambda_sc), float(lambda_ds), float(lambda_ss)
        self.beta, self.GNLL, self.usealldepth = bool(beta), bool(GNLL), bool(usealldepth)

    def forward(self, inputs, targets, target_depths=None, target_valid_depth=None, target_std=None, semantics=None, *,
                use_beta=True, add_depth=True, add_sem=True, labels_global=None, world=1):
        from . import _lib, _loss_lib as LL
        rgb0 = inputs["rgb_coarse"]
        _lib.require_device(rgb0)
        B, dev = rgb0.shape[0], rgb0.device
        if B == 0:
            raise ValueError("FusedTrainLoss: empty batch")
        f32 = lambda t: t.detach().contiguous().float()   # noqa: E731  (a constant of the loss)
        beta_on = self.beta and bool(use_beta)
        solar, sem = self.lambda_sc > 0, self.lambda_ss > 0
        form = LL.DEPTH_NONE
        if self.lambda_ds > 0:
            form = LL.DEPTH_ALL if self.usealldepth else (LL.DEPTH_SUBSET_GNLL if self.GNLL else LL.DEPTH_SUBSET_MSE)
        subset = form in (LL.DEPTH_SUBSET_MSE, LL.DEPTH_SUBSET_GNLL)
        g_depth, g_sem = form != LL.DEPTH_NONE and bool(add_depth), sem and bool(add_sem)
        g_weights = beta_on or (g_depth and form == LL.DEPTH_SUBSET_GNLL)
        keep = []   # every tensor a struct points to stays bound until the backward has run

        def hold(t):
            keep.append(t)
            return t.data_ptr()

        opts = LL.TrainLossOpts()
        opts.n_rays, opts.world = B, int(world)
        opts.flags = ((LL.LOSS_BETA if beta_on else 0) | (0 if add_depth else LL.LOSS_DEPTH_TERM_ONLY)
                      | (0 if add_sem else LL.LOSS_SEM_TERM_ONLY))
        opts.depth_form = form
        opts.lambda_sc, opts.lambda_ds, opts.lambda_ss = self.lambda_sc, self.lambda_ds, self.lambda_ss
        opts.ld_beta, opts.ld_td = 1, 2
        opts.target = hold(f32(targets))
        if form != LL.DEPTH_NONE:
            td = target_depths.detach().float()
            if td.dim() != 2 or td.shape[1] < 2:
                raise ValueError(f"FusedTrainLoss: target_depths is (B, 2) (depth, weight), got {tuple(td.shape)}")
            if td.stride(1) != 1:
                td = td.contiguous()
            opts.target_depth, opts.target_weight, opts.ld_td = hold(td), hold(td[:, 1:]), td.stride(0)
            if subset:
                if target_valid_depth is None:   # metrics.py:83-86: every ray has a prior
                    target_valid_depth = torch.ones(B, dtype=torch.int64, device=dev)
                opts.valid = hold(target_valid_depth.reshape(-1).long().contiguous())
                opts.target_std = hold(f32(target_std.reshape(-1)))
        if sem:
            labels = semantics.reshape(-1).long().contiguous()
            lg = labels if labels_global is None else labels_global.reshape(-1).long().contiguous()
            opts.labels, opts.labels_global, opts.n_global = hold(labels), hold(lg), lg.numel()
        passes, slots, counts = [], [], []
        for typ in ("coarse", "fine"):
            if typ == "fine" and "rgb_fine" not in inputs:
                break
            ps = LL.TrainLossPass()
            ps.n_samples, ps.ld_sun = 1, 1
            slot = dict.fromkeys(_PASS_INPUTS)
            slot["rgb"] = inputs[f"rgb_{typ}"].contiguous().float()
            ps.rgb = hold(slot["rgb"])
            S = None

            def samples(name, t):
                nonlocal S
                if S is None:
                    S = t.shape[1]
                elif t.shape[1] != S:
                    raise ValueError(f"FusedTrainLoss: {name}_{typ} has {t.shape[1]} samples per ray, expected {S}")

            if beta_on or subset:
                w = inputs[f"weights_{typ}"]
                samples("weights", w)
                w = w.contiguous().float() if g_weights else f32(w)
                ps.weights = hold(w)
                if g_weights:
                    slot["weights"] = w
            if subset:
                z = f32(inputs[f"z_vals_{typ}"])
                samples("z_vals", z)
                ps.z_vals = hold(z)
            if form != LL.DEPTH_NONE:
                d = inputs[f"depth_{typ}"].contiguous().float()
                ps.depth = hold(d)
                if g_depth:
                    slot["depth"] = d
            if solar:
                sun = inputs[f"sun_sc_{typ}"]
                samples("sun_sc", sun)
                sun, ps.ld_sun = _column(sun, S)
                ps.sun_sc = hold(sun)
                slot["sun_sc"] = sun
                ps.transparency_sc = hold(f32(inputs[f"transparency_sc_{typ}"]))
                ps.weights_sc = hold(f32(inputs[f"weights_sc_{typ}"]))
            if sem:
                lo = inputs[f"sem_logits_{typ}"].contiguous().float()
                opts.n_classes = lo.shape[1]
                ps.sem_logits = hold(lo)
                if g_sem:
                    slot["sem_logits"] = lo
            ps.n_samples = S or 1
            counts.append(S)
            passes.append(ps)
            slots += [slot[k] for k in _PASS_INPUTS]
        if len(passes) == 1:
            slots += [None] * len(_PASS_INPUTS)
        beta = None
        if beta_on:
            beta = inputs["beta_coarse"]
            if beta.shape[1] != counts[0] or (len(counts) > 1 and counts[1] != counts[0]):
                raise ValueError("FusedTrainLoss: the β form weights either pass's colour by beta_coarse; sample counts "
                                 f"beta_coarse {beta.shape[1]}, weights {counts}")
            beta, opts.ld_beta = _column(beta, counts[0])
            opts.beta = hold(beta)
        cfg = dict(opts=opts, passes=passes, keep=keep, device=dev)
        loss, block = _TrainLoss.apply(cfg, *slots, beta)
        terms = {}
        for p, typ in enumerate(("coarse", "fine")[:len(passes)]):
            names = ["color"] + (["logbeta"] if beta_on else []) + (["sc_term2", "sc_term3"] if solar else []) \
                + (["ds"] if form != LL.DEPTH_NONE else []) + (["ss"] if sem else [])
            for nm in names:
                terms[f"{typ}_{nm}"] = block[p * LL.PASS_TERMS + LL.TERM_SLOTS[nm]]
            for nm in ("mse", "psnr"):
                terms[f"{nm}_{typ}"] = block[p * LL.PASS_TERMS + LL.TERM_SLOTS[nm]]
        return loss, terms
