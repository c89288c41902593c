"""The kernels of the data-parallel training step (include/spnerf_amd_dp.h) — needs an MI355X.

* ``spnerf_dp_step_begin``: for world in {1, 2, 3} and a global batch of 48, every rank's launch on
  its own copy of the plan's state: the ranks' slices concatenated are the global batch and the
  permutation's slice, the clamp is the near / far of the global batch's first ray (bitwise), the
  global labels are ``sems[global_idx]``, ``cur`` is the row and the cursor moved by one; at
  world = 1 it writes what ``spnerf_train_step_begin`` writes; past the end, or against a plan of
  another batch size, nothing moves but the error word (every output holds its sentinel).
* ``spnerf_adam_step_dev_scaled`` on tensors of 1, 255 and 4 097 elements, one gradient holding
  subnormals: ``grad_scale = 1`` is bit-equal to ``spnerf_adam_step_dev``; ``grad_scale = 0.5`` is
  bit-equal to ``spnerf_adam_step_dev`` on gradients halved on the host beforehand (numpy: IEEE
  subnormals, round to nearest even).  Also with beta1 = 0, where ``exp_avg`` IS the scaled gradient,
  so a product rounded differently (or fused into the following subtraction) cannot hide."""
import ctypes

import numpy as np
import pytest
import torch

from spnerf_amd import _dp_lib, _lib, _train_lib, train

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, B, ROWS = 200, 48, 3


def _plan():
    """A hand-made plan: 3 rows of recognisable scalars and a permutation's first 3·48 entries."""
    rows = np.zeros(ROWS, train.ROW_DTYPE)
    for k in range(ROWS):
        rows[k] = (0.5 + k, 1e-3 * (k + 1), 2e-3 * (k + 1), 0.25 * (k + 1), 11 + k)
    g = torch.Generator().manual_seed(17)
    perm = torch.randperm(N, generator=g)[:ROWS * B].clone()
    rays = torch.randn(N, 11, generator=g)
    sems = torch.tensor(np.random.default_rng(2).choice([0, 1, 2, -100], size=N))
    return rows, perm, rays, sems


class Rank:
    """One rank's buffers, pre-filled with sentinels, two guard elements behind each."""

    def __init__(self, rows, perm, rank, world, plan_B=B):
        self.rank, self.world, self.b = rank, world, B // world
        self.rows = torch.from_numpy(rows.view(np.int64).copy()).to(DEV)
        self.perm = perm.to(DEV)
        self.state = torch.tensor([0, ROWS, plan_B, 0], dtype=torch.int64, device=DEV)
        self.cur = torch.full((3,), -1, dtype=torch.int64, device=DEV)
        self.idx = torch.full((self.b + 2,), -7, dtype=torch.int64, device=DEV)
        self.gidx = torch.full((B + 2,), -8, dtype=torch.int64, device=DEV)
        self.clamp = torch.full((4,), -9.0, dtype=torch.float32, device=DEV)
        self.labels = torch.full((B + 2,), -10, dtype=torch.int64, device=DEV)

    def outputs(self):
        return [t.clone() for t in (self.cur, self.idx, self.gidx, self.clamp, self.labels)]

    def begin(self, L, rays, sems):
        _lib.check(L.spnerf_dp_step_begin(_lib.ptr(self.state), _lib.ptr(self.rows), _lib.ptr(self.perm), _lib.ptr(self.cur),
                                          _lib.ptr(self.idx), _lib.ptr(self.gidx), B, self.rank, self.world,
                                          _lib.ptr(rays), rays.stride(0), _lib.ptr(self.clamp), _lib.ptr(sems),
                                          _lib.ptr(self.labels), _lib.stream_of(self.cur)), "dp_step_begin")
        torch.cuda.synchronize()


@pytest.mark.parametrize("world", [1, 2, 3])
def test_dp_step_begin_slices_the_global_batch(world):
    L = _dp_lib.lib()
    rows, perm, rays_h, sems_h = _plan()
    rays, sems = rays_h.to(DEV), sems_h.to(DEV)
    ranks = [Rank(rows, perm, r, world) for r in range(world)]
    for k in range(ROWS):
        want = perm[k * B:(k + 1) * B]
        for rk in ranks:
            rk.begin(L, rays, sems)
            assert rk.cur.cpu().numpy().tobytes() == rows[k].tobytes(), (k, rk.rank)
            assert rk.state.tolist() == [k + 1, ROWS, B, 0]
            assert torch.equal(rk.gidx[:B].cpu(), want) and rk.gidx[B:].tolist() == [-8, -8]
            assert torch.equal(rk.idx[:rk.b].cpu(), want[rk.rank * rk.b:(rk.rank + 1) * rk.b])
            assert rk.idx[rk.b:].tolist() == [-7, -7]
            # bitwise: compared as integers
            assert torch.equal(rk.clamp[:2].cpu().view(torch.int32), rays_h[want[0], 6:8].contiguous().view(torch.int32))
            assert rk.clamp[2:].tolist() == [-9.0, -9.0]
            assert torch.equal(rk.labels[:B].cpu(), sems_h[want]) and rk.labels[B:].tolist() == [-10, -10]
        assert torch.equal(torch.cat([rk.idx[:rk.b] for rk in ranks]), ranks[0].gidx[:B])
    # a fourth call: past the end, every output as it was
    for rk in ranks:
        before = rk.outputs()
        rk.begin(L, rays, sems)
        assert rk.state.tolist() == [ROWS, ROWS, B, _train_lib.ERR_PAST_END]
        assert all(torch.equal(x, y) for x, y in zip(rk.outputs(), before))


def test_dp_step_begin_at_world_1_is_train_step_begin():
    L = _dp_lib.lib()
    T = _train_lib.lib()
    rows, perm, rays_h, sems_h = _plan()
    rays, sems = rays_h.to(DEV), sems_h.to(DEV)
    rk = Rank(rows, perm, 0, 1)
    state = rk.state.clone()
    cur, idx = rk.cur.clone(), rk.idx.clone()
    for k in range(ROWS):
        rk.begin(L, rays, sems)
        _lib.check(T.spnerf_train_step_begin(_lib.ptr(state), _lib.ptr(rk.rows), _lib.ptr(rk.perm), _lib.ptr(cur),
                                             _lib.ptr(idx), B, _lib.stream_of(cur)), "train_step_begin")
        torch.cuda.synchronize()
        assert torch.equal(rk.cur, cur) and torch.equal(rk.idx, idx) and torch.equal(rk.state, state), k


def test_dp_step_begin_optional_outputs_and_untouched_sentinels():
    """global_idx, rays / clamp and sems / labels_global NULL: only cur, batch_idx, the cursor move;
    a fresh rank against sentinel-filled outputs that were never written stays at its sentinels on
    an error (nothing was ever stored there)."""
    L = _dp_lib.lib()
    rows, perm, rays_h, sems_h = _plan()
    rk = Rank(rows, perm, 1, 2)
    _lib.check(L.spnerf_dp_step_begin(_lib.ptr(rk.state), _lib.ptr(rk.rows), _lib.ptr(rk.perm), _lib.ptr(rk.cur),
                                      _lib.ptr(rk.idx), None, B, 1, 2, None, 0, None, None, None, _lib.stream_of(rk.cur)),
               "dp_step_begin")
    torch.cuda.synchronize()
    assert torch.equal(rk.idx[:24].cpu(), perm[24:48]) and rk.idx[24:].tolist() == [-7, -7]
    assert rk.cur.cpu().numpy().tobytes() == rows[0].tobytes() and rk.state.tolist() == [1, ROWS, B, 0]
    assert rk.gidx.tolist() == [-8] * (B + 2) and rk.clamp.tolist() == [-9.0] * 4 and rk.labels.tolist() == [-10] * (B + 2)


@pytest.mark.parametrize("cursor,err", [(0, _train_lib.ERR_BATCH), (ROWS, _train_lib.ERR_BATCH | _train_lib.ERR_PAST_END),
                                        (-1, _train_lib.ERR_PAST_END)], ids=["batch", "batch+past-end", "negative-cursor"])
def test_dp_step_begin_errors_leave_every_output(cursor, err):
    """A plan whose state->B is 24 (ERR_BATCH), or B right and the cursor outside the plan: nothing
    moves but the error word, on either rank."""
    L = _dp_lib.lib()
    rows, perm, rays_h, sems_h = _plan()
    rays, sems = rays_h.to(DEV), sems_h.to(DEV)
    for rank in (0, 1):
        rk = Rank(rows, perm, rank, 2, plan_B=24 if err & _train_lib.ERR_BATCH else B)
        rk.state[0] = cursor
        before = rk.outputs()
        rk.begin(L, rays, sems)
        assert rk.state.tolist() == [cursor, ROWS, 24 if err & _train_lib.ERR_BATCH else B, err]
        assert all(torch.equal(x, y) for x, y in zip(rk.outputs(), before))


def _lists(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


@pytest.mark.parametrize("beta1", [0.9, 0.0])
def test_scaled_adam_is_adam_on_scaled_gradients(beta1):
    L = _dp_lib.lib()
    T = _train_lib.lib()
    sizes = [1, 255, 4097]
    lr, b2, eps = 5e-4, 0.999, 1e-8
    g = torch.Generator().manual_seed(5)
    init = [torch.randn(n, generator=g) for n in sizes]
    tiny = np.float32(1.401298464324817e-45)          # the smallest subnormal
    numel = (ctypes.c_int64 * len(sizes))(*sizes)
    cur = torch.zeros(3, dtype=torch.int64, device=DEV)
    runs = ("plain", "scaled-1", "halved-first", "scaled-half")
    P = {k: [t.clone().to(DEV) for t in init] for k in runs}
    M = {k: [torch.zeros_like(t) for t in P[k]] for k in runs}
    V = {k: [torch.zeros_like(t) for t in P[k]] for k in runs}

    def step(run, grads, scale):
        args = (len(sizes), _lists(P[run]), _lists(grads), _lists(M[run]), _lists(V[run]), numel, _lib.ptr(cur), beta1, b2, eps)
        if scale is None:
            _lib.check(T.spnerf_adam_step_dev(*args, _lib.stream_of(cur)), "adam_step_dev")
        else:
            _lib.check(L.spnerf_adam_step_dev_scaled(*args, scale, _lib.stream_of(cur)), "adam_step_dev_scaled")

    for t in (1, 2):
        gh = [torch.randn(n, generator=g).numpy() * np.float32(10.0 ** (t - 2)) for n in sizes]
        # the 255-element gradient holds subnormals: odd multiples of the smallest one (halving
        # rounds them, to even), a few larger ones, both signs, and normal numbers in between
        sub = gh[1]
        sub[0:8] = tiny * np.array([1, 3, 5, 7, -1, -3, 2 ** 20 + 1, -(2 ** 22 + 3)], np.float32)
        sub[8] = np.float32(1.1754944e-38)             # the smallest normal: its half is subnormal
        sub[9] = np.float32(-1.1754945e-38)
        assert np.all(np.abs(sub[0:8]) > 0) and np.all(np.abs(sub[0:8]) < 1.1754944e-38)
        halved = [(x / np.float32(2.0)).astype(np.float32) for x in gh]      # IEEE on the host
        assert halved[1][0] == 0 and halved[1][1] == 2 * tiny and halved[1][2] == 2 * tiny and halved[1][3] == 4 * tiny
        gd = [torch.from_numpy(x.copy()).to(DEV) for x in gh]
        hd = [torch.from_numpy(x.copy()).to(DEV) for x in halved]
        row = np.zeros(1, train.ROW_DTYPE)
        ss, bc = train.adam_scalars(lr, beta1, b2, t)
        row[0] = (0.0, lr, ss, bc, t)
        cur.copy_(torch.from_numpy(row.view(np.int64).copy()))
        step("plain", gd, None)
        step("scaled-1", gd, 1.0)
        step("halved-first", hd, None)
        step("scaled-half", gd, 0.5)
        torch.cuda.synchronize()
        for a, b in (("plain", "scaled-1"), ("halved-first", "scaled-half")):
            for i, n in enumerate(sizes):
                for name, X in (("param", P), ("exp_avg", M), ("exp_avg_sq", V)):
                    assert torch.equal(X[a][i].view(torch.int32), X[b][i].view(torch.int32)), (t, a, b, n, name)
        if beta1 == 0.0:   # exp_avg is the scaled gradient itself, subnormals included (as values: -0 == 0)
            for i in range(len(sizes)):
                assert np.array_equal(M["scaled-half"][i].cpu().numpy(), halved[i]), sizes[i]
        # the gradients were read, not written
        assert all(np.array_equal(x.cpu().numpy().view(np.int32), y.view(np.int32)) for x, y in zip(gd, gh))
    assert not torch.equal(P["plain"][2], P["halved-first"][2])
