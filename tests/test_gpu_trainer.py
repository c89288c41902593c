"""spnerf_amd.train.Trainer — one HIP-graph replay per training step with the schedule on the device —
against a plain loop over what existed before it (needs an MI355X).

The model: W = 64, 8 layers, 3 classes, a t embedding; guided sampling, sc_lambda 0.05, depth,
semantic and β losses; 16 (+ 16 guided) samples, a synthetic dataset of 200 rays, batches of 48,
noise_std 1.0, max_train_steps 16, ds_drop 0.5, first_beta_epoch 1.  With 4 steps per epoch, 10 steps
cross the β switch (step 4), the depth drop (step 8), two learning-rate decays and two new
permutations (steps 5 and 9).

* ``test_trainer_equals_the_host_scalar_loop``: ten ``Trainer.step()`` calls leave every parameter,
  both Adam moments and every returned loss bit-equal to ten steps of ``reference_run`` below:
  ``render_rays`` with ``args.noise_std`` a host float decayed by 0.9, ``FusedTrainLoss`` with the
  host flags of main.py's rules, ``spnerf_amd.optim.Adam`` with its lr set by torch's ``StepLR``
  per epoch, ``dp.SharedSeedSampler`` and ``PhiloxRandom`` of the same seed.  With ``graph=True``
  (steps 1, 4, 8 run eagerly as the first of their loss form, 2, 5, 9 capture and replay, the rest
  only replay) and with ``graph=False``.
* ``test_resume_continues_bit_for_bit``: 6 steps, ``state_dict`` into a fresh ``Trainer``, 4 more
  steps: the same bits as the uninterrupted run.
* ``test_a_replay_step_issues_nothing_but_the_replay``: the suite does not use torch's sync debug
  mode on ROCm anywhere, so it is not relied on here; instead the property holds by construction:
  a step whose plan and loss form are current takes ``Trainer.step``'s first branch, which is
  ``graph.replay()`` and host bookkeeping.  The test replaces every other path of the trainer
  (``_slow_step``, ``_device_step``, ``_upload_plan``, ``_capture``) and the library handle with
  objects that raise, and runs such a step.
"""
import copy
import functools
import types

import numpy as np
import pytest
import torch

import golden_util as gu
import spnerf_amd
from spnerf_amd import dp, train

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, B, STEPS, SEED = 200, 48, 10, 7
SPE = N // B


def make_args():
    return types.SimpleNamespace(model="sp-nerf", n_samples=16, n_importance=0, guidedsample=True, sc_lambda=0.05,
                                 beta=True, first_beta_epoch=1, depth=True, ds_lambda=1.0, ds_drop=0.5, GNLL=False,
                                 usealldepth=False, sem=True, ss_lambda=0.04, ss_drop=1, margin=1e-4, stdscale=1.0,
                                 chunk=5120, noise_std=1.0, lr=5e-4, batch_size=B, max_train_steps=16,
                                 t_embbeding_tau=4, t_embbeding_vocab=8, num_sem_classes=3)


@functools.lru_cache(maxsize=None)
def dataset():
    g = torch.Generator().manual_seed(21)
    rays = torch.tensor(gu.synthetic_rays(N, 5))
    far = rays[:, 7]
    d = {"rays": rays, "rgbs": torch.rand(N, 3, generator=g),
         "depths": torch.stack([far * (0.3 + 0.4 * torch.rand(N, generator=g)), 0.2 + 0.8 * torch.rand(N, generator=g)], 1),
         "valid_depth": (torch.rand(N, generator=g) < 0.7).long(),
         "depth_std": far * (0.01 + 0.05 * torch.rand(N, generator=g)),
         "sems": torch.tensor(np.random.default_rng(4).choice([0, 1, 2, -100], size=N, p=[0.4, 0.3, 0.2, 0.1])),
         "ts": (torch.arange(N) % 8).reshape(N, 1)}
    return {k: v.to(DEV).contiguous() for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def initial_models(precision):
    torch.manual_seed(3)
    m = spnerf_amd.SPNeRF(num_sem_classes=3, layers=8, feat=64, mapping=True, t_embedding_dims=4, beta=True, sem=True,
                          precision=precision)
    return {"coarse": m, "t": torch.nn.Embedding(8, 4)}


def make_models(precision):
    return {k: copy.deepcopy(m).to(DEV) for k, m in initial_models(precision).items()}


@functools.lru_cache(maxsize=None)
def reference_run(precision):
    """Ten steps of the plain loop; (losses, parameters, exp_avg, exp_avg_sq), computed once."""
    a, R = make_args(), dataset()
    models = make_models(precision)
    models["coarse"].use_flat_grads()
    params = [p for m in models.values() for p in m.parameters()]
    opt = spnerf_amd.optim.Adam(params, lr=a.lr)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.9)
    sampler = dp.SharedSeedSampler(N, B, 0, 1, seed=SEED, device=DEV)
    src = spnerf_amd.PhiloxRandom(seed=SEED)
    floss = spnerf_amd.FusedTrainLoss(lambda_sc=a.sc_lambda, beta=True, lambda_ds=a.ds_lambda, lambda_ss=a.ss_lambda)
    ds_drop, ss_drop = np.round(a.ds_drop * a.max_train_steps), np.round(a.ss_drop * a.max_train_steps)   # main.py:30,35
    losses, train_steps = [], 0
    for _ in range(STEPS):
        train_steps += 1
        _, idx = sampler.next()
        bt = {k: v[idx] for k, v in R.items()}
        opt.zero_grad(set_to_none=True)
        with spnerf_amd.random_source(src):
            res = spnerf_amd.render_rays(models, a, bt["rays"], bt["ts"].squeeze(), semantics=bt["sems"].squeeze(),
                                         mode="train", valid_depth=bt["valid_depth"], target_depths=bt["depths"],
                                         target_std=bt["depth_std"])
            loss, _ = floss(res, bt["rgbs"], bt["depths"], bt["valid_depth"], bt["depth_std"], bt["sems"],
                            use_beta=not (train_steps // SPE < a.first_beta_epoch),          # main.py:150
                            add_depth=bool(train_steps < ds_drop), add_sem=bool(train_steps < ss_drop))   # :163,172
            loss.backward()
        a.noise_std *= 0.9                                                                    # main.py:155
        opt.step()
        if train_steps % SPE == 0:
            sched.step()                                                                      # per epoch
        losses.append(loss.detach().clone())
    torch.cuda.synchronize()
    assert all(torch.isfinite(x) for x in losses)
    return (losses, [p.detach().clone() for p in params], [opt.state[p]["exp_avg"].clone() for p in params],
            [opt.state[p]["exp_avg_sq"].clone() for p in params])


def assert_same_state(tr, ref, what):
    _, params, m, v = ref
    torch.cuda.synchronize()
    assert len(tr.params) == len(params)
    names = [f"{k}.{n}" for k, mod in tr.models.items() for n, _ in mod.named_parameters()]
    for i, n in enumerate(names):
        assert torch.equal(tr.params[i], params[i]), (what, "parameter", n)
        assert torch.equal(tr.exp_avg[i], m[i]), (what, "exp_avg", n)
        assert torch.equal(tr.exp_avg_sq[i], v[i]), (what, "exp_avg_sq", n)


@pytest.mark.parametrize("graph,precision", [(True, "bf16"), (False, "bf16"), (True, "fp32")],
                         ids=["graph-bf16", "eager-bf16", "graph-fp32"])
def test_trainer_equals_the_host_scalar_loop(graph, precision):
    ref = reference_run(precision)
    tr = train.Trainer(make_models(precision), make_args(), dataset(), seed=SEED, graph=graph)
    assert tr.spe == SPE
    for t in range(STEPS):
        loss = tr.step()
        assert loss.is_cuda and loss.dim() == 0
        assert torch.equal(loss, ref[0][t]), (t + 1, float(loss), float(ref[0][t]))
    assert_same_state(tr, ref, "graph" if graph else "eager")
    tr.check_error()
    assert tr.counts["plan_upload"] == 3
    if graph:
        assert (tr.counts["eager"], tr.counts["capture"], tr.counts["replay"]) == (3, 3, 7)
    else:
        assert (tr.counts["eager"], tr.counts["capture"], tr.counts["replay"]) == (10, 0, 0)
    # the moved parameters are not the initial ones, and the schedule did decay on the device
    start = [p for m in make_models(precision).values() for p in m.parameters()]
    assert sum(not torch.equal(p, q) for p, q in zip(tr.params, start)) > len(start) // 2
    row = np.frombuffer(tr.cur.cpu().numpy().tobytes(), train.ROW_DTYPE)[0]
    x = 1.0
    for _ in range(STEPS - 1):
        x *= 0.9
    assert row["step"] == STEPS and row["noise_std"] == np.float32(x) and row["lr"] == np.float32(5e-4 * 0.9 * 0.9)


def test_resume_continues_bit_for_bit():
    ref = reference_run("bf16")
    first = train.Trainer(make_models("bf16"), make_args(), dataset(), seed=SEED)
    first.fit(6)
    sd = first.state_dict()
    assert sd["global_step"] == 6 and sd["plan_cursor"] == 2 and sd["philox_step"] == 5
    second = train.Trainer(make_models("bf16"), make_args(), dataset(), seed=SEED)
    second.load_state_dict(sd)
    for t in range(6, STEPS):
        loss = second.step()
        assert torch.equal(loss, ref[0][t]), t + 1
    assert_same_state(second, ref, "resumed")
    second.check_error()
    with pytest.raises(ValueError, match="seed"):
        train.Trainer(make_models("bf16"), make_args(), dataset(), seed=SEED + 1).load_state_dict(sd)


def test_a_replay_step_issues_nothing_but_the_replay():
    ref = reference_run("bf16")
    tr = train.Trainer(make_models("bf16"), make_args(), dataset(), seed=SEED)
    tr.fit(2)                      # step 1 eager, step 2 the capture and its replay
    assert tr.counts == {"replay": 1, "eager": 1, "capture": 1, "plan_upload": 1}

    def refuse(*a, **k):
        raise AssertionError("a replay step left Trainer.step's replay branch")

    class Refusing:
        def __getattr__(self, name):
            refuse()

    tr._slow_step = tr._device_step = tr._upload_plan = tr._capture = tr._adam = refuse
    tr.lib, tr.gather = Refusing(), refuse
    loss = tr.step()               # step 3: same epoch, same loss form
    assert tr.counts["replay"] == 2 and tr.global_step == 3
    assert torch.equal(loss, ref[0][2])
    assert tr.state.tolist() == [3, SPE, B, 0]      # the device cursor moved with it
