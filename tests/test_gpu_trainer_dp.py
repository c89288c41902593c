"""spnerf_amd.train.Trainer with world = 2 — the data-parallel training step — against a plain
data-parallel loop over the pieces that existed before it, and against one process training the
whole batch (needs an MI355X).

Two ranks share cuda:0 over gloo (RCCL refuses two ranks on one device), so ``collectives="host"``:
the graph holds step-begin through backward, the bucket all-reduces, the t embedding's all-reduce
and the scaled Adam follow each replay.  The shapes are tests/test_gpu_trainer.py's: W = 64, 8
layers, 3 classes, a t embedding, 16 + 16 guided samples, 200 rays, a GLOBAL batch of 48 (24 per
rank, 4 steps per epoch), so 10 steps cross the β switch, the depth drop, two learning-rate decays
and two permutations.

One spawn of two workers per (graph, precision) serves every test that reads it (``runs``); each
rank writes an ``.npz``.  A rank that dies ends ``mp.spawn``; a rank that waits for a dead one is
ended by the process group's timeout (``dp.pg_timeout_seconds``).

* ``test_dp_trainer_equals_the_dp_host_loop``: ten ``Trainer(world=2).step()`` calls leave every
  parameter, both moments and every local loss bit-equal to ten steps of ``dp_host_loop`` below
  (``SharedSeedSampler(rank, world)``, ``PhiloxRandom(ray_offset=rank·b)``, ``render_rays`` with the
  global batch's first ray as ``clamp_near_far`` and a host ``noise_std``, ``FusedTrainLoss`` with
  ``labels_global`` / ``world``, ``dp.allreduce_grads``, ``spnerf_amd.optim.Adam`` under ``StepLR``), on
  both ranks, and the two ranks bit-equal to each other.  Bit equality is the bar because the
  arithmetic and its order are the same by construction: a sum of two is commutative, the bucketed
  and the flat all-reduce agree bitwise (tests/test_gpu_dp.py), and at world = 2 scaling by 0.5
  inside Adam rounds like dividing by 2 first.
* ``test_dp_step_matches_single_process``: after ONE step, the 2-rank all-reduced flat gradient
  times 1/2 against the single-process ``Trainer(world=1)`` gradient of the whole batch, by
  tests/test_gpu_dp.py's measure and bounds for this comparison (whole-flat relative L2 < 1e-4 fp32,
  5e-3 bf16; the worst tensor of >= 64 elements < 10 times that); the mean of the ranks' losses
  within 1e-4 (relative) of the single-process loss in fp32.  One step only: Adam's sign-like first
  update turns rounding-level gradient differences near zero into parameter differences of order lr.
* ``test_dp_resume_and_world_mismatch``: 6 steps, ``state_dict`` into a fresh 2-rank trainer, 4
  more: the bits of 10 uninterrupted steps; loading it into a world = 1 trainer raises ValueError.
* ``test_global_loss``: ``global_loss(loss)`` is the mean of the two ranks' losses, bitwise, on both.
"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

WORLD, STEPS = 2, 10


def dp_host_loop(base, rank, world, precision):
    """Ten data-parallel steps written from the pieces; (losses, params, exp_avg, exp_avg_sq)."""
    import spnerf_amd
    from spnerf_amd import dp
    a, R = base.make_args(), base.dataset()
    N, B, SPE, DEV = base.N, base.B, base.SPE, base.DEV
    b = B // world
    models = base.make_models(precision)
    models["coarse"].use_flat_grads()
    params = [p for m in models.values() for p in m.parameters()]
    opt = spnerf_amd.optim.Adam(params, lr=a.lr)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.9)
    sampler = dp.SharedSeedSampler(N, B, rank, world, seed=base.SEED, device=DEV)
    src = spnerf_amd.PhiloxRandom(seed=base.SEED, ray_offset=rank * b)
    floss = spnerf_amd.FusedTrainLoss(lambda_sc=a.sc_lambda, beta=True, lambda_ds=a.ds_lambda, lambda_ss=a.ss_lambda)
    ds_drop, ss_drop = np.round(a.ds_drop * a.max_train_steps), np.round(a.ss_drop * a.max_train_steps)   # main.py:30,35
    losses, train_steps = [], 0
    for _ in range(STEPS):
        train_steps += 1
        gidx, idx = sampler.next()
        bt = {k: v[idx] for k, v in R.items()}
        opt.zero_grad(set_to_none=True)
        with spnerf_amd.random_source(src):
            res = spnerf_amd.render_rays(models, a, bt["rays"], bt["ts"].squeeze(), semantics=bt["sems"].squeeze(),
                                         mode="train", valid_depth=bt["valid_depth"], target_depths=bt["depths"],
                                         target_std=bt["depth_std"], clamp_near_far=R["rays"][gidx[0], 6:8])
            loss, _ = floss(res, bt["rgbs"], bt["depths"], bt["valid_depth"], bt["depth_std"], bt["sems"],
                            use_beta=not (train_steps // SPE < a.first_beta_epoch),          # main.py:150
                            add_depth=bool(train_steps < ds_drop), add_sem=bool(train_steps < ss_drop),   # :163,172
                            labels_global=R["sems"][gidx], world=world)
            loss.backward()
        a.noise_std *= 0.9                                                                    # main.py:155
        dp.allreduce_grads(params, world)
        opt.step()
        if train_steps % SPE == 0:
            sched.step()                                                                      # per epoch
        losses.append(loss.detach().clone())
    torch.cuda.synchronize()
    return (losses, [p.detach().clone() for p in params], [opt.state[p]["exp_avg"].clone() for p in params],
            [opt.state[p]["exp_avg_sq"].clone() for p in params])


def _pack(prefix, losses, params, m, v):
    out = {f"{prefix}|loss": torch.stack([x.reshape(()) for x in losses]).cpu().numpy()}
    for name, ts in (("p", params), ("m", m), ("v", v)):
        for i, t in enumerate(ts):
            out[f"{prefix}|{name}{i}"] = t.detach().cpu().numpy()
    return out


def rank_run(rank, world, graph, precision, with_resume):
    """Everything one rank computes for the tests, as a dict of host arrays."""
    import torch.distributed as dist

    import test_gpu_trainer as base
    from spnerf_amd import train
    pg = dist.group.WORLD

    def trainer():
        return train.Trainer(base.make_models(precision), base.make_args(), base.dataset(), seed=base.SEED, graph=graph,
                             world=world, group=pg, collectives="host")

    out = {}
    tr = trainer()
    assert tr.rank == rank and tr.b == base.B // world and tr.spe == base.SPE and tr.collectives == "host"
    losses, global_losses = [], []
    for t in range(STEPS):
        loss = tr.step()
        assert loss.is_cuda and loss.dim() == 0
        losses.append(loss.clone())
        global_losses.append(tr.global_loss(loss))
        if t == 0:   # the all-reduce's SUM of step 1, before the next backward overwrites it
            out["flat_sum_step1"] = tr.models["coarse"]._flat_grad.cpu().numpy().copy()
    tr.check_error()
    out.update(_pack("trainer", losses, tr.params, tr.exp_avg, tr.exp_avg_sq))
    out["global_loss"] = torch.stack(global_losses).cpu().numpy()
    out["counts"] = np.array([tr.counts[k] for k in ("eager", "capture", "replay", "plan_upload")])
    out["state"] = tr.state.cpu().numpy()
    del tr
    out.update(_pack("loop", *dp_host_loop(base, rank, world, precision)))
    if with_resume:
        first = trainer()
        first.fit(6)
        sd = first.state_dict()
        assert sd["world"] == world and sd["global_step"] == 6 and sd["plan_cursor"] == 2
        del first
        second = trainer()
        second.load_state_dict(sd)
        losses = [second.step().clone() for _ in range(6, STEPS)]
        second.check_error()
        out.update(_pack("resumed", losses, second.params, second.exp_avg, second.exp_avg_sq))
        del second
        single = train.Trainer(base.make_models(precision), base.make_args(), base.dataset(), seed=base.SEED, graph=graph)
        try:
            single.load_state_dict(sd)
            out["world_mismatch"] = np.array("loaded")
        except ValueError as e:
            out["world_mismatch"] = np.array(f"ValueError: {e}")
    return out


def _worker(rank, world, port, outdir, graph, precision, with_resume):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (here, os.path.dirname(here)):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    from spnerf_amd import dp
    torch.cuda.set_device(0)
    dp.init_from_env("gloo")
    out = rank_run(rank, world, graph, precision, with_resume)
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), **out)
    dist.barrier()
    dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """``runs(graph, precision)`` → the two ranks' results, each configuration spawned once."""
    cache = {}

    def get(graph, precision):
        key = (graph, precision)
        if key not in cache:
            d = tmp_path_factory.mktemp(f"dp_{'graph' if graph else 'eager'}_{precision}")
            with_resume = key == (True, "bf16")
            mp.spawn(_worker, args=(WORLD, _free_port(), str(d), graph, precision, with_resume), nprocs=WORLD, join=True)
            cache[key] = [dict(np.load(d / f"rank{r}.npz")) for r in range(WORLD)]
        return cache[key]

    return get


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _state_keys(run, prefix):
    return sorted(k for k in run if k.startswith(prefix + "|") and not k.endswith("|loss"))


@pytest.mark.parametrize("graph,precision", [(True, "bf16"), (False, "bf16"), (True, "fp32")],
                         ids=["graph-bf16", "eager-bf16", "graph-fp32"])
def test_dp_trainer_equals_the_dp_host_loop(runs, graph, precision):
    ranks = runs(graph, precision)
    for r, run in enumerate(ranks):
        assert np.all(np.isfinite(run["loop|loss"])) and run["loop|loss"].shape == (STEPS,)
        for t in range(STEPS):
            assert _same_bits(run["trainer|loss"][t], run["loop|loss"][t]), (r, t + 1, run["trainer|loss"][t], run["loop|loss"][t])
        keys = _state_keys(run, "trainer")
        assert len(keys) == len(_state_keys(run, "loop")) and len(keys) % 3 == 0 and keys
        for k in keys:
            assert _same_bits(run[k], run["loop|" + k.split("|")[1]]), (r, k)
        eager, capture, replay, uploads = run["counts"].tolist()
        assert uploads == 3
        assert (eager, capture, replay) == ((3, 3, 7) if graph else (10, 0, 0))
        assert run["state"].tolist() == [2, 4, 48, 0]          # the cursor, the plan of the GLOBAL batch, no error
    for k in _state_keys(ranks[0], "trainer"):
        assert _same_bits(ranks[0][k], ranks[1][k]), k         # the ranks hold the same model
    # the ranks trained different rays: their local losses differ; and the parameters did move
    assert not np.array_equal(ranks[0]["trainer|loss"], ranks[1]["trainer|loss"])
    import test_gpu_trainer as base
    start = [p.detach().numpy() for m in base.initial_models(precision).values() for p in m.parameters()]
    moved = sum(not np.array_equal(ranks[0][f"trainer|p{i}"], s) for i, s in enumerate(start))
    assert moved > len(start) // 2


@pytest.mark.parametrize("precision,tol", [("fp32", 1e-4), ("bf16", 5e-3)])
def test_dp_step_matches_single_process(runs, precision, tol):
    import test_gpu_trainer as base
    from spnerf_amd import train
    ranks = runs(True, precision)
    assert _same_bits(ranks[0]["flat_sum_step1"], ranks[1]["flat_sum_step1"])
    got = ranks[0]["flat_sum_step1"].astype(np.float64) * 0.5
    tr = train.Trainer(base.make_models(precision), base.make_args(), base.dataset(), seed=base.SEED, graph=True)
    loss = tr.step()
    ref = tr.models["coarse"]._flat_grad.cpu().numpy().astype(np.float64)
    loss = float(loss)
    assert got.shape == ref.shape and np.any(ref)
    total = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    worst, off = {}, 0
    for n, p in tr.models["coarse"].named_parameters():
        g, r = got[off:off + p.numel()], ref[off:off + p.numel()]
        off += p.numel()
        if r.size >= 64 and np.any(r):
            worst[n] = np.linalg.norm(g - r) / max(np.linalg.norm(r), 1e-30)
    assert off == ref.size
    mean_loss = 0.5 * (float(ranks[0]["trainer|loss"][0]) + float(ranks[1]["trainer|loss"][0]))
    print(precision, f"flat {total:.2e}", sorted(worst.items(), key=lambda kv: -kv[1])[:4],
          f"loss {mean_loss:.8g} vs {loss:.8g} ({abs(mean_loss - loss) / abs(loss):.2e})")
    assert total < tol, total
    assert max(worst.values()) < 10 * tol, worst
    if precision == "fp32":
        assert abs(mean_loss - loss) <= 1e-4 * abs(loss), (mean_loss, loss)


def test_dp_resume_and_world_mismatch(runs):
    for r, run in enumerate(runs(True, "bf16")):
        for t in range(6, STEPS):
            assert _same_bits(run["resumed|loss"][t - 6], run["trainer|loss"][t]), (r, t + 1)
        keys = _state_keys(run, "resumed")
        assert len(keys) == len(_state_keys(run, "trainer"))
        for k in keys:
            assert _same_bits(run[k], run["trainer|" + k.split("|")[1]]), (r, k)
        msg = str(run["world_mismatch"])
        assert msg.startswith("ValueError") and "world" in msg, msg


def test_global_loss(runs):
    ranks = runs(True, "bf16")
    mean = ((ranks[0]["trainer|loss"] + ranks[1]["trainer|loss"]) / np.float32(2)).astype(np.float32)
    assert ranks[0]["trainer|loss"].dtype == np.float32
    for run in ranks:
        assert _same_bits(run["global_loss"], mean)
