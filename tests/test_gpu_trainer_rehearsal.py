"""spnerf_amd.train.Trainer's ``collectives="graph"`` path on one GPU (needs an MI355X): a one-rank
``nccl`` group on cuda:0, so that ``Trainer(world=1, group=pg)`` runs the whole data-parallel
machinery — ``spnerf_dp_step_begin``, the shared clamp and global labels from their fixed buffers,
the bucket all-reduces behind the backward's marks CAPTURED into the step's graph (identity
all-reduces with one rank), the t embedding's all-reduce, the scaled Adam with scale 1 — and must
leave the bits of the plain single-GPU ``Trainer``: tests/test_gpu_trainer.py's ``reference_run``
(parameters, both moments, every loss) over the same 10 steps.  The counts show that every step
after the first two of a loss form is one replay.

In a file of its own: RCCL refuses two ranks on one device, so this is the only test of the
captured collectives, and it can be judged on its own."""
import os
import socket

import pytest
import torch
import torch.distributed as dist

import test_gpu_trainer as base
from spnerf_amd import train

pytestmark = pytest.mark.gpu


@pytest.fixture
def one_rank_nccl():
    assert not dist.is_initialized()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    old = {k: os.environ.get(k) for k in ("MASTER_ADDR", "MASTER_PORT")}
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(base.DEV))
    try:
        yield dist.group.WORLD
    finally:
        torch.cuda.synchronize()
        dist.destroy_process_group()
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_one_rank_rehearsal_of_the_captured_collectives_equals_the_plain_trainer(one_rank_nccl):
    ref = base.reference_run("bf16")
    tr = train.Trainer(base.make_models("bf16"), base.make_args(), base.dataset(), seed=base.SEED, graph=True, world=1,
                       group=one_rank_nccl, collectives="graph")
    assert tr.dp and tr.collectives == "graph" and tr.rank == 0 and tr.b == base.B and tr.grad_scale == 1.0
    assert len(tr.buckets) == 1 and len(tr.buckets[0].buckets) > 1 and len(tr.loose) == 1
    seen = []
    for t in range(base.STEPS):
        loss = tr.step()
        assert torch.equal(loss, ref[0][t]), (t + 1, float(loss), float(ref[0][t]))
        seen.append((tr.counts["eager"], tr.counts["capture"], tr.counts["replay"]))
    base.assert_same_state(tr, ref, "rehearsal")
    tr.check_error()
    assert tr.global_loss(loss).item() == float(ref[0][-1])
    # steps 1, 4, 8 are the first of their loss form (eager), 2, 5, 9 capture and replay, every
    # other step is one replay and nothing else
    assert seen == [(1, 0, 0), (1, 1, 1), (1, 1, 2), (2, 1, 2), (2, 2, 3), (2, 2, 4), (2, 2, 5), (3, 2, 5), (3, 3, 6), (3, 3, 7)]
    assert tr.counts["plan_upload"] == 3 and not tr._tail_after_replay
    # "auto" picks the captured collectives for nccl
    assert train.Trainer(base.make_models("bf16"), base.make_args(), base.dataset(), seed=base.SEED, world=1,
                         group=one_rank_nccl).collectives == "graph"
