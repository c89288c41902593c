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
    """The reference's training loop on one GPU.

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
    clamp's first ray is the batch's first ray."""

    def __init__(self, models, args, dataset_tensors, *, seed: int = 0, precision: str | None = None,
                 graph: bool = True, world: int = 1, betas=(0.9, 0.999), eps: float = 1e-8):
        from . import _train_lib
        from .spnerf import SPNeRF
        if world > 1:
            raise NotImplementedError("Trainer: data parallelism (world > 1) is not part of the trainer yet")
        self._tl = _train_lib
        self.lib = _train_lib.lib()
        self.models = models
        self.args = a = types.SimpleNamespace(**vars(args))
        self.graph_mode = bool(graph)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        B = self.B = int(a.batch_size)
        if B > int(getattr(a, "chunk", B)):
            raise NotImplementedError(f"Trainer: batch_size {B} > chunk {a.chunk}: the batch is rendered in one call")
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
        self.src = PhiloxRandom(seed=seed)
        self.gather = BatchGather(self.fields, B)
        # fixed device addresses of the step: the current row, the plan's state, the plan itself
        self.cur = torch.zeros(ROW_DTYPE.itemsize // 8, dtype=torch.int64, device=dev)
        self.noise_std_dev = self.cur.view(torch.float32)[0:1]          # &cur->noise_std
        self.state = torch.zeros(4, dtype=torch.int64, device=dev)      # spnerf_train_state
        self.plan_rows = torch.zeros(self.spe * (ROW_DTYPE.itemsize // 8), dtype=torch.int64, device=dev)
        self.perm = torch.zeros(self.spe * B, dtype=torch.int64, device=dev)
        self.batch_idx = torch.zeros(B, dtype=torch.int64, device=dev)
        self.one = torch.ones((), device=dev)
        self.global_step = 0          # steps done
        self._plan_epoch = None       # epoch of the uploaded plan
        self._host_plan = None
        self._graph = None
        self._graph_form = None
        self._graph_keep = None       # what the captured graph writes into and must outlive it
        self._static_loss = None
        self._warm = set()            # loss forms that have run eagerly once
        self.counts = {"replay": 0, "eager": 0, "capture": 0, "plan_upload": 0}

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
        _lib.check(self.lib.spnerf_adam_step_dev(n, arr([self.params[i] for i in have]), arr(grads),
                                                 arr([self.exp_avg[i] for i in have]),
                                                 arr([self.exp_avg_sq[i] for i in have]), numel, _lib.ptr(self.cur),
                                                 self.betas[0], self.betas[1], self.eps, _lib.stream_of(self.cur)),
                   "adam_step_dev")

    def _device_step(self, form):
        """Everything a step does on the device, in stream order — the body of the captured graph:
        schedule + batch (step_begin), gather, render, loss, backward, Adam."""
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
                "plan_cursor": self.global_step % self.spe, "seed": self.schedule.seed}

    def load_state_dict(self, sd: dict) -> None:
        if sd["seed"] != self.schedule.seed:
            raise ValueError(f"Trainer.load_state_dict: saved with seed {sd['seed']}, this trainer has {self.schedule.seed}")
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
