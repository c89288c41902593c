"""The host side of the trainer's epoch plan (spnerf_amd.train.make_plan / Schedule / loss_form)
against what the host-scalar path computes: torch's StepLR, csrc/adam.hip's host expressions, the
``noise_std *= 0.9`` loop, dp.SharedSeedSampler's batches and main.py's drop / β rules.  No GPU."""
import math
import types

import numpy as np
import torch

from spnerf_amd import dp, train


def test_lr_per_step_is_steplr_stepped_per_epoch():
    lr0, spe, B = 5e-4, 7, 4
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([p], lr=lr0)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.9)
    s = train.Schedule(spe * B + 3, B, lr0)
    assert s.steps_per_epoch == spe
    for epoch in range(3):
        plan = s.plan(epoch)
        assert plan.n_steps == spe and plan.first_step == epoch * spe + 1
        want = np.float32(opt.param_groups[0]["lr"])
        for k in range(spe):
            assert plan.rows["lr"][k] == want, (epoch, k)            # exact float equality
            assert plan.rows["step"][k] == epoch * spe + k + 1
        opt.step()
        sched.step()
    # the stateless entry gives the same rows
    again = train.make_plan(2, dataset_len=spe * B + 3, batch_size=B, lr0=lr0)
    assert again.rows.tobytes() == plan.rows.tobytes() and torch.equal(again.perm, plan.perm)


def test_adam_scalars_are_the_host_codes():
    lr, b1, b2 = 5e-4, 0.9, 0.999
    for t in (1, 2, 10, 1000):
        bc1, bc2 = 1.0 - math.pow(b1, t), 1.0 - math.pow(b2, t)      # adam.hip: std::pow in double
        ss, bc = train.adam_scalars(lr, b1, b2, t)
        assert ss == np.float32(lr / bc1) and bc == np.float32(math.sqrt(bc2))
    # in a plan: steps 1, 2, 10 (epoch 0 of 12 steps) and 1 000 (epoch 83, with that epoch's lr)
    s = train.Schedule(12 * 3, 3, lr)
    plan = s.plan(0)
    for t in (1, 2, 10):
        ss, bc = train.adam_scalars(lr, b1, b2, t)
        assert plan.rows["adam_step_size"][t - 1] == ss and plan.rows["adam_bc2_sqrt"][t - 1] == bc
    plan = s.plan(999 // 12)
    k = 999 % 12
    assert plan.rows["step"][k] == 1000
    lr_e = lr
    for _ in range(999 // 12):
        lr_e = lr_e * 0.9
    ss, bc = train.adam_scalars(lr_e, b1, b2, 1000)
    assert plan.rows["adam_step_size"][k] == ss and plan.rows["adam_bc2_sqrt"][k] == bc
    assert plan.rows["lr"][k] == np.float32(lr_e)


def test_noise_std_is_the_decay_loop():
    s = train.Schedule(5 * 8, 8, 5e-4, noise_std0=1.0)
    x = 1.0
    for epoch in range(4):
        plan = s.plan(epoch)
        for k in range(5):
            assert plan.rows["noise_std"][k] == np.float32(x), (epoch, k)   # the float the host passes (c_float)
            x *= 0.9                                                         # main.py:155
    assert train.Schedule(40, 8, 5e-4, noise_std0=0.0).plan(3).rows["noise_std"].tolist() == [0.0] * 5
    # asking for an earlier epoch again replays from the seed
    assert s.plan(1).rows["noise_std"][0] == np.float32(_decayed(1.0, 5))


def _decayed(x, n):
    for _ in range(n):
        x *= 0.9
    return x


def test_batches_are_the_shared_seed_samplers():
    n, B, seed = 50, 16, 11
    sampler = dp.SharedSeedSampler(n, B, 0, 1, seed)
    s = train.Schedule(n, B, 5e-4, seed=seed)
    assert s.steps_per_epoch == 3                       # the tail of 2 rays is dropped
    for epoch in range(3):
        plan = s.plan(epoch)
        assert plan.perm.dtype == torch.int64 and plan.perm.numel() == 3 * B
        for k in range(3):
            g, mine = sampler.next()                     # re-permutes when the sampler does
            assert torch.equal(plan.batch(k), g) and torch.equal(mine, g), (epoch, k)
    other = train.make_plan(0, dataset_len=n, batch_size=B, lr0=5e-4, seed=seed + 1)
    assert not torch.equal(other.perm, s.plan(0).perm)


def test_loss_form_boundaries_follow_main_py():
    a = types.SimpleNamespace(beta=True, first_beta_epoch=2, depth=True, ds_drop=0.25, sem=True, ss_drop=1,
                              max_train_steps=40)
    spe = 6
    forms = {t: train.loss_form(t, a, spe) for t in range(1, 41)}
    # depth: train_steps < round(0.25 * 40) = 10, the strict inequality the reference writes
    assert [t for t in forms if forms[t][1]] == list(range(1, 10))
    # semantic: train_steps < 40
    assert [t for t in forms if forms[t][2]] == list(range(1, 40))
    # β once get_current_epoch(train_steps) = train_steps // steps_per_epoch reaches first_beta_epoch
    assert [t for t in forms if forms[t][0]] == list(range(12, 41))
    # np.round rounds halves to even, like the reference's np.round: 0.5 * 5 = 2.5 -> 2
    b = types.SimpleNamespace(beta=False, depth=True, ds_drop=0.5, sem=False, ss_drop=1, max_train_steps=5)
    assert [t for t in range(1, 6) if train.loss_form(t, b, spe)[1]] == [1]
    assert train.loss_form(1, b, spe) == (False, True, False)
    # a model without the head never takes the form
    c = types.SimpleNamespace(beta=False, depth=False, ds_drop=1, sem=False, ss_drop=1, max_train_steps=5)
    assert train.loss_form(1, c, spe) == (False, False, False)
