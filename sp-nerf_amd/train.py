"""Training a scene — the reference trainer's step and schedule (``NeRF_pl.training_step`` and
``configure_optimizers``, main.py:95-106,125-186) with ONE replay of one HIP graph per step.

The schedule of the reference:

* Adam with ``StepLR(step_size=1, gamma=0.9)`` stepped per epoch (main.py:97-99, utils.py:318);
* ``noise_std *= 0.9`` after every step (main.py:155);
* the depth term dropped at ``round(ds_drop · max_train_steps)``, the semantic term at ``ss_drop``
  (main.py:30,35,163,172);
* the plain colour loss while ``epoch < first_beta_epoch``, then the β form (main.py:150).

Everything that changes per step lives on the device.  The host computes each step's scalars in
double, exactly as the host-scalar path does, and uploads them once per epoch with the epoch's
permutation (``EpochPlan``); the captured step starts with ``spnerf_train_step_begin`` (the step's
row to a fixed address, its index slice into the gather's index buffer, the cursor advanced), the
composites read ``noise_std`` and Adam its two bias-correction scalars from that address
(include/spnerf_amd_train.h).  A replay therefore covers the schedule, the batch, gather, render,
loss, backward and Adam: no per-step host-to-device copy, host scalar or host sync.  The loss form
changes at most three times in a run (β on, depth dropped, semantic dropped); it stays a host flag
of ``FusedTrainLoss`` and the trainer re-captures its graph at those boundaries.
"""
from __future__ import annotations

import ctypes
import math
import types
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .dp import BatchGather
from .losses import FusedTrainLoss
from .rng import PhiloxRandom, random_source

# one row of the plan: spnerf_train_step_scalars (include/spnerf_amd_train.h), 24 bytes
ROW_DTYPE = np.dtype([("noise_std", "<f4"), ("lr", "<f4"), ("adam_step_size", "<f4"), ("adam_bc2_sqrt", "<f4"),
                      ("step", "<i8")])
FIELDS = ("rays", "rgbs", "depths", "valid_depth", "depth_std", "sems", "ts")


@dataclass
class EpochPlan:
    """The host side of one epoch's plan: ``rows[k]`` are the scalars of the epoch's step k (global
    step ``first_step + k``), ``perm[k·B : (k+1)·B]`` its ray indices."""
    epoch: int
    first_step: int          # global step t (>= 1) of row 0
    n_steps: int
    batch_size: int
    rows: np.ndarray         # (n_steps,) ROW_DTYPE
    perm: torch.Tensor       # (n_steps · batch_size,) int64, CPU

    def batch(self, k: int) -> torch.Tensor:
        return self.perm[k * self.batch_size:(k + 1) * self.batch_size]


def adam_scalars(lr: float, beta1: float, beta2: float, t: int):
    """(step_size, bc2_sqrt) of Adam step ``t`` as csrc/adam.hip's host code computes them: in
    double, rounded to float once."""
    bc1 = 1.0 - math.pow(beta1, t)
    bc2 = 1.0 - math.pow(beta2, t)
    return np.float32(lr / bc1), np.float32(math.sqrt(bc2))


class Schedule:
    """The per-step scalars and permutations of a run, epoch after epoch.

    ``steps_per_epoch = dataset_len // batch_size`` and ``epoch = step // steps_per_epoch``
    (utils.get_epoch_number_from_train_step).  The learning rate follows ``StepLR(step_size=1,
    gamma)``'s own recurrence (``lr *= gamma`` per epoch, in double), ``noise_std`` the trainer's
    ``x *= 0.9`` per step (Python double, rounded to float where it is passed), the Adam scalars
    ``adam_scalars``.  The permutations are those of ``dp.SharedSeedSampler(n, B, 0, 1, seed)``: one
    ``torch.randperm`` from a CPU generator seeded once, drawn anew when the next batch would run
    past the end, so every permutation serves ``steps_per_epoch`` batches and its tail is dropped."""

    def __init__(self, dataset_len: int, batch_size: int, lr0: float, noise_std0: float = 0.0, seed: int = 0,
                 betas=(0.9, 0.999), gamma: float = 0.9, noise_decay: float = 0.9):
        if batch_size < 1 or dataset_len < batch_size:
            raise ValueError(f"Schedule: batch_size {batch_size} must be in [1, dataset_len = {dataset_len}]")
        self.n, self.B = int(dataset_len), int(batch_size)
        self.steps_per_epoch = self.n // self.B
        self.lr0, self.noise_std0, self.seed = float(lr0), float(noise_std0), int(seed)
        self.betas, self.gamma, self.noise_decay = (float(betas[0]), float(betas[1])), float(gamma), float(noise_decay)
        self._rewind()

    def _rewind(self):
        self._epoch = 0                      # the epoch the carried values below belong to
        self._gen = torch.Generator(device="cpu").manual_seed(self.seed)
        self._lr, self._noise = self.lr0, self.noise_std0

    def _advance(self, with_perm: bool):
        """The carried values of the next epoch; the current epoch's permutation when asked."""
        perm = torch.randperm(self.n, generator=self._gen)
        spe = self.steps_per_epoch
        t0 = self._epoch * spe + 1
        rows = None
        if with_perm:
            rows = np.zeros(spe, ROW_DTYPE)
        x = self._noise
        for k in range(spe):
            if with_perm:
                ss, bc = adam_scalars(self._lr, self.betas[0], self.betas[1], t0 + k)
                rows[k] = (np.float32(x), np.float32(self._lr), ss, bc, t0 + k)
            x *= self.noise_decay
        plan = None
        if with_perm:
            plan = EpochPlan(self._epoch, t0, spe, self.B, rows, perm[:spe * self.B].clone())
        self._noise = x
        self._lr = self._lr * self.gamma     # StepLR.get_lr: group["lr"] * gamma
        self._epoch += 1
        return plan

    def plan(self, epoch: int) -> EpochPlan:
        """The plan of ``epoch`` (>= 0).  Consecutive epochs cost one permutation each; going back
        replays the generator from its seed."""
        if epoch < 0:
            raise ValueError("Schedule.plan: negative epoch")
        if epoch < self._epoch:
            self._rewind()
        while self._epoch < epoch:
            self._advance(False)
        return self._advance(True)


def make_plan(epoch: int, *, dataset_len: int, batch_size: int, lr0: float, noise_std0: float = 0.0, seed: int = 0,
              betas=(0.9, 0.999), gamma: float = 0.9) -> EpochPlan:
    """The plan of one epoch from scratch (``Schedule(...).plan(epoch)``)."""
    return Schedule(dataset_len, batch_size, lr0, noise_std0, seed, betas, gamma).plan(epoch)


def loss_form(t: int, args, steps_per_epoch: int):
    """(use_beta, add_depth, add_sem) of global step ``t`` (>= 1, the reference's ``train_steps`` after
    its increment) by main.py's rules: the β form once ``t // steps_per_epoch`` has reached
    ``first_beta_epoch`` (:150), the depth term while ``t < round(ds_drop · max_train_steps)`` (:30,163),
    the semantic term while ``t < round(ss_drop · max_train_steps)`` (:35,172)."""
    use_beta = bool(getattr(args, "beta", False)) and not (t // steps_per_epoch < getattr(args, "first_beta_epoch", 2))
    add_depth = bool(getattr(args, "depth", False)) and t < float(np.round(args.ds_drop * args.max_train_steps))
    add_sem = bool(getattr(args, "sem", False)) and t < float(np.round(args.ss_drop * args.max_train_steps))
    return use_beta, add_depth, add_sem


def _parameters(models):
    """utils.get_parameters: the models' parameters in the dictionary's order."""
    out = []
    for m in models.values():
        out += list(m.parameters())
    return out


class Trainer:
    """The reference's training loop on one GPU, or data-parallel on N.

    ``models``: the ``{"coarse", ["fine"], ["t"]}`` dictionary ``render_rays`` takes; ``args``: the
    reference's ``Train_parser`` names (``lr``, ``batch_size``, ``max_train_steps``, ``noise_std``,
    ``n_samples``, ``n_importance``, ``guidedsample``, ``sc_lambda``, ``beta``, ``first_beta_epoch``,
    ``depth``, ``ds_lambda``, ``ds_drop``, ``GNLL``, ``usealldepth``, ``sem``, ``ss_lambda``,
    ``ss_drop``, ``chunk``), read at construction and not modified; ``dataset_tensors``: the
    HBM-resident per-ray fields ``BatchGather`` takes — ``rays`` (N, 11), ``rgbs`` (N, 3) and, as the
    flags need them, ``depths`` (N, 2), ``valid_depth`` (N,), ``depth_std`` (N,), ``sems`` (N,),
    ``ts`` (N,) or (N, 1) int64 — as ``spnerf_amd.dataset`` builds them.

    ``step()`` runs one training step and returns the loss as a device scalar without a host
    sync; with ``graph=True`` a step is one graph replay, except the first step of a loss form (run
    eagerly, which also warms every kernel the capture will record) and the second (the capture,
    then its replay).  ``graph=False`` runs every step eagerly through the same device-resident
    scalars.  ``fit(n)`` runs ``n`` steps.  The plan of an epoch is uploaded when its first step is
    due; the previous epoch's error word is read then (one host sync per epoch).

    The batch is rendered in one ``render_rays`` call (``batch_size <= chunk``), so the guided
    clamp's first ray is the batch's first ray.

    Data parallelism (``world > 1``, one process per GPU inside a ``torch.distributed`` group, see
    ``dp.init_from_env``): ``args.batch_size`` stays the GLOBAL batch B and each rank trains
    ``b = B // world`` rays of it.  Every rank builds the same ``Schedule`` from the same seed, so
    plan and permutation agree without a collective.  The step starts with ``spnerf_dp_step_begin``
    (include/spnerf_amd_dp.h): the row, this rank's slice of the global batch, the global batch's
    first ray's near / far (the guided clamp all ranks share) and the global batch's labels (the
    CE's denominator) into fixed buffers; the draws are keyed by the global ray id
    (``PhiloxRandom(ray_offset=rank·b)``).  The gradients are all-reduced (SUM) in ``dp.GradBuckets``
    per SPNeRF plus one small all-reduce for parameters outside a flat buffer (the ``t`` embedding),
    and ``spnerf_adam_step_dev_scaled`` multiplies by 1/world as it loads them: no pass divides.
    ``collectives="graph"`` (nccl only) captures the bucket all-reduces behind the backward's marks
    with the rest of the step — still one replay per step; ``"host"`` (gloo; any backend) ends the
    graph with the backward and issues the all-reduces and Adam after each replay: a few host calls
    more, no host sync of the trainer's; ``"auto"`` = ``"graph"`` for nccl, else ``"host"``.
    ``world=1`` with an explicit ``group`` rehearses that machinery with one rank (identity
    all-reduces, scale 1); ``world=1`` without a group is the single-GPU path.  ``rank`` is the
    group's.  ``step()`` returns this rank's loss; ``global_loss(loss)`` all-reduces it."""

    def __init__(self, models, args, dataset_tensors, *, seed: int = 0, precision: str | None = None,
                 graph: bool = True, world: int = 1, rank: int = 0, group=None, collectives: str = "auto",
                 betas=(0.9, 0.999), eps: float = 1e-8):
        # what needs neither the library nor a device comes first
        world, rank = int(world), int(rank)
        if world < 1:
            raise ValueError(f"Trainer: world = {world} < 1")
        if int(args.batch_size) % world:
            raise ValueError(f"Trainer: the global batch_size {int(args.batch_size)} does not divide over {world} ranks")
        if collectives not in ("auto", "graph", "host"):
            raise ValueError(f"Trainer: collectives must be 'auto', 'graph' or 'host', got {collectives!r}")
        self.dp = world > 1 or group is not None      # the data-parallel machinery (one rank: a rehearsal)
        self.world, self.group, self.collectives = world, group, None
        if self.dp:
            rank = self._join_group(world, rank, group, collectives)
        elif rank != 0:
            raise ValueError(f"Trainer: rank {rank} with world = 1")
        self.rank = rank
        from . import _train_lib
        from .spnerf import SPNeRF
        self._tl = _train_lib
        self.lib = _train_lib.lib()
        self.models = models
        self.args = a = types.SimpleNamespace(**vars(args))
        self.graph_mode = bool(graph)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        B = self.B = int(a.batch_size)          # the GLOBAL batch (the reference's batch_size)
        b = self.b = B // world                 # this rank's rays per step
        if b > int(getattr(a, "chunk", b)):
            raise NotImplementedError(f"Trainer: batch_size {b} > chunk {a.chunk}: the batch is rendered in one call")
        self.fields = {k: dataset_tensors[k] for k in FIELDS if k in dataset_tensors}
        for k in ("rays", "rgbs"):
            if k not in self.fields:
                raise ValueError(f"Trainer: dataset_tensors lacks {k!r}")
        _lib.require_device(*self.fields.values())
        self.dev = dev = self.fields["rays"].device
        need = (["depths", "valid_depth", "depth_std"] if (getattr(a, "depth", False) or a.guidedsample) else []) \
            + (["sems"] if getattr(a, "sem", False) else []) + (["ts"] if getattr(a, "beta", False) else [])
        for k in need:
            if k not in self.fields:
                raise ValueError(f"Trainer: these flags need dataset_tensors[{k!r}]")
        self.nets = [m for m in models.values() if isinstance(m, SPNeRF)]
        for m in self.nets:
            if precision is not None:
                m.set_precision(precision)
            m.use_flat_grads()
        self.params = _parameters(models)
        for p in self.params:
            if p.dtype != torch.float32 or p.device != dev or not p.is_contiguous():
                raise _lib.SpnerfError("Trainer: parameters must be contiguous fp32 tensors on the dataset's device")
        self.exp_avg = [torch.zeros_like(p) for p in self.params]
        self.exp_avg_sq = [torch.zeros_like(p) for p in self.params]
        self.schedule = Schedule(self.fields["rays"].shape[0], B, a.lr, a.noise_std, seed, self.betas)
        self.spe = self.schedule.steps_per_epoch
        self.floss = FusedTrainLoss(lambda_sc=a.sc_lambda, beta=bool(getattr(a, "beta", False)),
                                    lambda_ds=a.ds_lambda if getattr(a, "depth", False) else 0.0,
                                    GNLL=bool(getattr(a, "GNLL", False)), usealldepth=bool(getattr(a, "usealldepth", False)),
                                    lambda_ss=a.ss_lambda if getattr(a, "sem", False) else 0.0)
        # draws are keyed by the GLOBAL ray id: rank r's rays are rows r·b.. of the global batch
        self.src = PhiloxRandom(seed=seed, ray_offset=rank * b)
        self.gather = BatchGather(self.fields, b)
        # fixed device addresses of the step: the current row, the plan's state, the plan itself
        self.cur = torch.zeros(ROW_DTYPE.itemsize // 8, dtype=torch.int64, device=dev)
        self.noise_std_dev = self.cur.view(torch.float32)[0:1]          # &cur->noise_std
        self.state = torch.zeros(4, dtype=torch.int64, device=dev)      # spnerf_train_state
        self.plan_rows = torch.zeros(self.spe * (ROW_DTYPE.itemsize // 8), dtype=torch.int64, device=dev)
        self.perm = torch.zeros(self.spe * B, dtype=torch.int64, device=dev)
        self.batch_idx = torch.zeros(b, dtype=torch.int64, device=dev)
        self.one = torch.ones((), device=dev)
        if self.dp:
            self._init_dp()
        self.global_step = 0          # steps done
        self._plan_epoch = None       # epoch of the uploaded plan
        self._host_plan = None
        self._graph = None
        self._graph_form = None
        self._graph_keep = None       # what the captured graph writes into and must outlive it
        self._static_loss = None
        self._warm = set()            # loss forms that have run eagerly once
        self.counts = {"replay": 0, "eager": 0, "capture": 0, "plan_upload": 0}

    # ------------------------------------------------------------------ data parallelism
    def _join_group(self, world: int, rank: int, group, collectives: str) -> int:
        """Check the process group against ``world`` and settle ``collectives``; this rank."""
        import torch.distributed as dist
        if group is None:
            if not dist.is_initialized():
                raise NotImplementedError(f"Trainer: world = {world} without a torch.distributed process group is not "
                                          "implemented: start one process per GPU, call dp.init_from_env() and pass "
                                          "world (and group)")
            group = self.group = dist.group.WORLD
        elif rank != 0:
            raise ValueError("Trainer: an explicit rank goes without a group (the group knows this process's rank)")
        if dist.get_world_size(group) != world:
            raise ValueError(f"Trainer: world = {world} but the process group has {dist.get_world_size(group)} ranks")
        backend = str(dist.get_backend(group))
        if collectives == "graph" and backend != "nccl":
            raise ValueError(f"Trainer: collectives='graph' needs the nccl backend (RCCL's all-reduce can be captured "
                             f"into the step's graph), this group's is {backend!r}: use 'host'")
        self.collectives = ("graph" if backend == "nccl" else "host") if collectives == "auto" else collectives
        return dist.get_rank(group)

    def _init_dp(self) -> None:
        """The data-parallel step's fixed device buffers, its bindings and the gradient buckets."""
        from . import _dp_lib
        from .dp import GradBuckets
        self._dl = _dp_lib
        _dp_lib.lib()          # the same handle as self.lib with the dp signatures applied; no fallback
        rays = self.fields["rays"]
        if rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] < 8 or not rays.is_contiguous():
            raise ValueError("Trainer: dataset_tensors['rays'] must be a contiguous (N, >= 8) fp32 tensor")
        self.clamp = torch.zeros(2, dtype=torch.float32, device=self.dev)    # near / far of the global batch's first ray
        self.labels_global = None
        self._sems = None
        if getattr(self.args, "sem", False):
            sems = self.fields["sems"]
            if sems.dtype != torch.int64 or sems.numel() != rays.shape[0] or not sems.is_contiguous():
                raise ValueError("Trainer: dataset_tensors['sems'] must be a contiguous int64 tensor of N labels")
            self._sems = sems
            self.labels_global = torch.zeros(self.B, dtype=torch.int64, device=self.dev)
        self.buckets = [GradBuckets(m, self.world, self.group) for m in self.nets]
        in_nets = {id(p) for m in self.nets for p in m.parameters()}
        self.loose = [p for p in self.params if id(p) not in in_nets]        # e.g. the t embedding
        # (float)(1 / world), rounded once: Adam multiplies the all-reduce's SUM by it as it loads it
        self.grad_scale = float(np.float32(1.0 / self.world))
        # the marks are one event set per device: with one net every bucket can go behind its own
        # mark; with two, the buckets wait for the whole backward instead
        self._overlap = len(self.nets) == 1
        self._tail_after_replay = False   # collectives == "host": reduce + Adam follow each replay

    def _reduce(self, overlap: bool) -> None:
        """All-reduce (SUM) of every gradient: each net's flat gradient in buckets — behind their
        backward marks when ``overlap``, else behind the whole compute stream — and the parameters
        outside a flat buffer in one more small all-reduce.  The SUM stays: Adam scales it."""
        from . import dp
        flats = []
        for m, bk in zip(self.nets, self.buckets):
            flat = dp._shared_flat([p.grad for p in m.parameters()]) if all(p.grad is not None for p in m.parameters()) \
                else None
            if flat is None:
                raise _lib.SpnerfError("Trainer: a data-parallel step needs every SPNeRF parameter's gradient in the "
                                       "model's flat buffer (use_flat_grads, no frozen parameter)")
            bk.launch(flat, overlap=overlap and self._overlap, force=True)
            flats.append(flat)
        for bk, flat in zip(self.buckets, flats):
            bk.finish(flat, force=True, scale=False)
        dp.allreduce_grads(self.loose, self.world, self.group, scale=False, force=True)

    def global_loss(self, loss: torch.Tensor) -> torch.Tensor:
        """The loss of the GLOBAL batch (the reference's ``train/loss``) from this rank's ``step()``
        result: a copy all-reduced (SUM) and divided by ``world`` — the colour, solar and depth terms
        are sums over rays divided by the batch size and the CE is already rescaled by the loss
        kernel, so the ranks' losses average to it.  A collective: every rank calls it.  Not part of
        the step; with one rank and no group, a copy."""
        out = loss.detach().clone()
        if self.dp:
            import torch.distributed as dist
            dist.all_reduce(out, op=dist.ReduceOp.SUM, group=self.group)
            if self.world > 1:
                out.div_(self.world)
        return out

    # ------------------------------------------------------------------ the plan, once per epoch
    def check_error(self) -> None:
        """Read the plan's error word (a host sync) and raise if a step began outside its plan."""
        err = int(self.state[3].item())
        if err:
            what = [s for bit, s in ((self._tl.ERR_PAST_END, "a step began past the end of its epoch's plan"),
                                     (self._tl.ERR_BATCH, "a step's batch size differs from the plan's")) if err & bit]
            raise _lib.SpnerfError(f"Trainer: device error word {err}: " + "; ".join(what))

    def _upload_plan(self, epoch: int, cursor: int = 0) -> None:
        if self._plan_epoch is not None:
            self.check_error()
        plan = self.schedule.plan(epoch)
        self.plan_rows.copy_(torch.from_numpy(plan.rows.view(np.int64).copy()))
        self.perm.copy_(plan.perm)
        self.state.copy_(torch.tensor([cursor, plan.n_steps, self.B, 0], dtype=torch.int64))
        self._plan_epoch, self._host_plan = epoch, plan
        self.counts["plan_upload"] += 1

    # ------------------------------------------------------------------ one step's device work
    def _adam(self) -> None:
        have = [i for i, p in enumerate(self.params) if p.grad is not None]
        if not have:
            return
        n = len(have)
        grads = [self.params[i].grad if self.params[i].grad.is_contiguous() else self.params[i].grad.contiguous()
                 for i in have]
        arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])   # noqa: E731
        numel = (ctypes.c_int64 * n)(*[self.params[i].numel() for i in have])
        if self.dp:   # the gradients hold the all-reduce's SUM: scaled by 1/world as they are loaded
            _lib.check(self.lib.spnerf_adam_step_dev_scaled(n, arr([self.params[i] for i in have]), arr(grads),
                                                            arr([self.exp_avg[i] for i in have]),
                                                            arr([self.exp_avg_sq[i] for i in have]), numel,
                                                            _lib.ptr(self.cur), self.betas[0], self.betas[1], self.eps,
                                                            self.grad_scale, _lib.stream_of(self.cur)),
                       "adam_step_dev_scaled")
            return
        _lib.check(self.lib.spnerf_adam_step_dev(n, arr([self.params[i] for i in have]), arr(grads),
                                                 arr([self.exp_avg[i] for i in have]),
                                                 arr([self.exp_avg_sq[i] for i in have]), numel, _lib.ptr(self.cur),
                                                 self.betas[0], self.betas[1], self.eps, _lib.stream_of(self.cur)),
                   "adam_step_dev")

    def _dp_device_step(self, form, tail: bool = True):
        """The data-parallel step in stream order: spnerf_dp_step_begin (the row, this rank's slice,
        the shared clamp, the global labels), gather, render, loss, backward — and with ``tail`` the
        gradient all-reduces (buckets behind the backward's marks) and the scaled Adam.  Without it
        (the graph of ``collectives="host"``) ``_host_tail`` follows each replay."""
        from .rendering import render_rays
        from .spnerf import device_noise_std
        a = self.args
        use_beta, add_depth, add_sem = form
        rays_all = self.fields["rays"]
        _lib.check(self.lib.spnerf_dp_step_begin(_lib.ptr(self.state), _lib.ptr(self.plan_rows), _lib.ptr(self.perm),
                                                 _lib.ptr(self.cur), _lib.ptr(self.batch_idx), None, self.B, self.rank,
                                                 self.world, _lib.ptr(rays_all), rays_all.stride(0), _lib.ptr(self.clamp),
                                                 _lib.ptr(self._sems), _lib.ptr(self.labels_global),
                                                 _lib.stream_of(self.cur)), "dp_step_begin")
        for p in self.params:
            p.grad = None
        bt = self.gather(self.batch_idx)
        rays, rgbs = bt["rays"], bt["rgbs"]
        depths, valid, dstd = bt.get("depths"), bt.get("valid_depth"), bt.get("depth_std")
        sems = bt["sems"].reshape(-1) if getattr(a, "sem", False) else None
        ts = bt["ts"].reshape(-1) if getattr(a, "beta", False) else None
        lkw = {"labels_global": self.labels_global, "world": self.world} if sems is not None else {}
        # The buckets go behind their backward marks where that pays: inside the capture of
        # collectives="graph" (there the marks are the graph's edges) and in every step of
        # graph=False.  The few eager steps of graph=True reduce behind the whole backward instead, so
        # that a mark event is only ever recorded and waited for inside captures, or only outside.
        overlap = tail and self._overlap and (torch.cuda.is_current_stream_capturing() or not self.graph_mode)
        if overlap:
            _lib.grad_marks_arm(True)     # the backward records the buckets' marks
        try:
            with random_source(self.src), device_noise_std(self.noise_std_dev):
                res = render_rays(self.models, a, rays, ts, semantics=sems, mode="train", valid_depth=valid,
                                  target_depths=depths, target_std=dstd, clamp_near_far=self.clamp)
                loss, _ = self.floss(res, rgbs, depths, valid, dstd, sems, use_beta=use_beta, add_depth=add_depth,
                                     add_sem=add_sem, **lkw)
                loss.backward(self.one)
            if tail:
                self._reduce(overlap=overlap)
        finally:
            if overlap:
                _lib.grad_marks_arm(False)
        if tail:
            self._adam()
        return loss.detach()

    def _host_tail(self) -> None:
        """What follows a replay of the ``collectives="host"`` graph on the stream: the buckets behind
        the whole replay, the loose parameters' all-reduce, Adam — a few host calls, no host sync of
        the trainer's own."""
        self._reduce(overlap=False)
        self._adam()

    def _device_step(self, form):
        """Everything a step does on the device, in stream order — the body of the captured graph:
        schedule + batch (step_begin), gather, render, loss, backward, Adam."""
        if self.dp:
            return self._dp_device_step(form)
        from .rendering import render_rays
        from .spnerf import device_noise_std
        a = self.args
        use_beta, add_depth, add_sem = form
        _lib.check(self.lib.spnerf_train_step_begin(_lib.ptr(self.state), _lib.ptr(self.plan_rows), _lib.ptr(self.perm),
                                                    _lib.ptr(self.cur), _lib.ptr(self.batch_idx), self.B,
                                                    _lib.stream_of(self.cur)), "train_step_begin")
        for p in self.params:
            p.grad = None      # the backward writes the gradients (the flat buffer is zeroed in stream order)
        bt = self.gather(self.batch_idx)
        rays, rgbs = bt["rays"], bt["rgbs"]
        depths, valid, dstd = bt.get("depths"), bt.get("valid_depth"), bt.get("depth_std")
        sems = bt["sems"].reshape(-1) if getattr(a, "sem", False) else None          # main.py:132
        ts = bt["ts"].reshape(-1) if getattr(a, "beta", False) else None             # main.py:131
        with random_source(self.src), device_noise_std(self.noise_std_dev):
            res = render_rays(self.models, a, rays, ts, semantics=sems, mode="train", valid_depth=valid,
                              target_depths=depths, target_std=dstd)
            loss, _ = self.floss(res, rgbs, depths, valid, dstd, sems, use_beta=use_beta, add_depth=add_depth,
                                 add_sem=add_sem)
            loss.backward(self.one)   # d loss / d loss = 1 from a static tensor (no fill launch per step)
        self._adam()
        return loss.detach()

    def _capture(self, form) -> None:
        torch.cuda.synchronize(self.dev)
        for p in self.params:
            p.grad = None
        g = torch.cuda.CUDAGraph()
        if self.dp and self.collectives == "host":
            # the graph ends with the backward; the collectives and Adam follow each replay
            with torch.cuda.graph(g):
                self._static_loss = self._dp_device_step(form, tail=False)
            self._tail_after_replay = True
        else:   # with collectives="graph" the bucket all-reduces are captured behind their marks
            with torch.cuda.graph(g):
                self._static_loss = self._device_step(form)
        # the packed-weight buffers the capture wrote into live exactly as long as the graph
        self._graph_keep = [m.release_graph_packs() for m in self.nets]
        self._graph, self._graph_form = g, form
        self.counts["capture"] += 1

    def _drop_graph(self) -> None:
        self._graph = self._graph_form = self._graph_keep = self._static_loss = None
        for p in self.params:
            p.grad = None      # views of the dropped graph's pool

    # ------------------------------------------------------------------ the public loop
    def step(self) -> torch.Tensor:
        """One training step; the loss as a 0-d device tensor (with ``graph=True`` the graph's static
        output: read it before the next step).  A step that replays issues nothing but the replay."""
        t = self.global_step + 1
        if self._graph is not None and self._plan_epoch == (t - 1) // self.spe and \
                self._graph_form == loss_form(t, self.args, self.spe):
            self._graph.replay()
            if self.dp and self._tail_after_replay:
                self._host_tail()
            self.counts["replay"] += 1
            self.global_step = t
            return self._static_loss
        return self._slow_step(t)

    def _slow_step(self, t: int) -> torch.Tensor:
        """A step that is not a plain replay: a new epoch's plan, a new loss form, eager mode."""
        epoch = (t - 1) // self.spe
        if self._plan_epoch != epoch:
            self._upload_plan(epoch, (t - 1) % self.spe)
        form = loss_form(t, self.args, self.spe)
        if self._graph is not None and self._graph_form != form:
            self._drop_graph()
        if not self.graph_mode or form not in self._warm:
            loss = self._device_step(form)
            self._warm.add(form)
            self.counts["eager"] += 1
        else:
            if self._graph is None:
                self._capture(form)
            self._graph.replay()
            if self.dp and self._tail_after_replay:
                self._host_tail()
            self.counts["replay"] += 1
            loss = self._static_loss
        self.global_step = t
        return loss

    def fit(self, n_steps: int) -> torch.Tensor:
        """``n_steps`` steps (the per-epoch plan uploads included); the last step's loss."""
        loss = None
        for _ in range(int(n_steps)):
            loss = self.step()
        return loss

    def learning_rate(self) -> float:
        """The learning rate of the uploaded plan's epoch (utils.get_learning_rate); before the first
        step, the initial one."""
        return float(self.args.lr) if self._host_plan is None else float(self._host_plan.rows["lr"][0])

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self) -> dict:
        """Parameters, Adam moments, global step, Philox step and plan cursor (a host sync): a fresh
        ``Trainer`` of the same construction that loads it continues bit for bit."""
        return {"models": {k: {n: v.detach().clone() for n, v in m.state_dict().items()} for k, m in self.models.items()},
                "exp_avg": [t.clone() for t in self.exp_avg], "exp_avg_sq": [t.clone() for t in self.exp_avg_sq],
                "global_step": self.global_step, "philox_step": self.src.sync_host_step(),
                "plan_cursor": self.global_step % self.spe, "seed": self.schedule.seed, "world": self.world}

    def load_state_dict(self, sd: dict) -> None:
        if sd["seed"] != self.schedule.seed:
            raise ValueError(f"Trainer.load_state_dict: saved with seed {sd['seed']}, this trainer has {self.schedule.seed}")
        if sd.get("world", 1) != self.world:   # the Philox ray offsets and the ranks' slices would differ
            raise ValueError(f"Trainer.load_state_dict: saved with world = {sd.get('world', 1)}, this trainer has "
                             f"{self.world}")
        if sd["plan_cursor"] != sd["global_step"] % self.spe:
            raise ValueError("Trainer.load_state_dict: the plan cursor does not match this dataset and batch size")
        self._drop_graph()
        with torch.no_grad():
            for k, m in self.models.items():
                for n, v in m.state_dict().items():
                    v.copy_(sd["models"][k][n])       # in place: the parameters keep their addresses
            for dst, src in zip(self.exp_avg + self.exp_avg_sq, sd["exp_avg"] + sd["exp_avg_sq"]):
                dst.copy_(src)
        self.global_step = int(sd["global_step"])
        self.src.reset_step(int(sd["philox_step"]))
        self._plan_epoch = None     # the next step uploads its epoch's plan with the saved cursor
